"""Cost of decoding straight to integer PCM of the caller's layout (alac_hip_decode_int) against alac_hip_decode,
alac_hip_decode_float and a decode followed by the conversion a torch user writes today for the same tensor:
    python tools/decode_int_timing.py [--out result.json]
For 10 000 and 125 000 synthetic packets (BASELINE configs[1] / the configs[3] shard), 16-bit and 24-bit stereo, every
packet independent, all in one process:
  decode            alac_hip_decode into a device buffer (interleaved integer bytes)
  decode_float      alac_hip_decode_float into a float32 [2, T] device tensor
  int32_planar      alac_hip_decode_int into an int32 [2, T] tensor, left-justified: the bytes, sites and store widths of
                    decode_float.  The bar: its median lies within decode_float's [min, max] of this run, widened by its own
  int32_interleaved alac_hip_decode_int into an int32 [T, 2] tensor, left-justified (one store per sample)
  int16_planar      16-bit stream only: alac_hip_decode_int into an int16 [2, T] tensor (8-byte stores)
  packed3           24-bit stream only: alac_hip_decode_int into packed 3-byte containers [T, 2, 3] (three byte stores per
                    sample; the identity descriptor, so what it competes with is decode itself)
  composed_*        alac_hip_decode, then view / unpack the bytes, shift, transpose and .contiguous() in torch, for the tensor
                    of the column of the same name.  The bar: every decode_int layout beats its composed route
Times are milliseconds between two events on the context's stream around one call, inputs and outputs on the device and
allocated once.  A figure is the median over 7 rounds of the median of 10 calls (3 warm-up calls in front of the first round);
"spread" is the smallest and the largest round."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import alac_amd  # noqa: E402

ROUNDS = 7


def rounds_ms(ctx, fn, reps=10, warm=3, rounds=ROUNDS):
    for _ in range(warm):
        fn()
    ctx.synchronize()
    out = []
    for _ in range(rounds):
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ctx.stream)
            fn()
            b.record(ctx.stream)
            b.synchronize()
            times.append(a.elapsed_time(b))
        out.append(statistics.median(times))
    return {"ms": statistics.median(out), "spread_ms": [min(out), max(out)]}


def samples(pcm, depth):
    """decode's bytes -> the left-justified int32 container of every sample, flat and interleaved: what a caller of decode()
    writes"""
    if depth == 16:
        return pcm.view(torch.int16).to(torch.int32) << 16
    b = pcm.view(-1, 3).to(torch.int32)  # 3-byte containers: no 24-bit dtype, so unpack by hand
    return (b[:, 0] << 8) | (b[:, 1] << 16) | (b[:, 2] << 24)


def composed(pcm, depth, channels, column):
    if column == "int32_planar":
        return samples(pcm, depth).view(-1, channels).t().contiguous()
    if column == "int32_interleaved":
        return samples(pcm, depth).view(-1, channels)
    assert column == "int16_planar" and depth == 16
    return pcm.view(torch.int16).view(-1, channels).t().contiguous()


def measure(ctx, n, depth):
    fmt = alac_amd.make_format(4096, depth, 2, 44100)
    d_pcm = ctx.synth_pcm(0, n, fmt)
    cookie = ctx.magic_cookie(fmt)
    r = {"packets": n, "bit_depth": depth, "channels": 2}
    columns = {"int32_planar": dict(dtype=torch.int32, layout="planar"),
               "int32_interleaved": dict(dtype=torch.int32, layout="interleaved")}
    if depth == 16:
        columns["int16_planar"] = dict(dtype=torch.int16, layout="planar")
    else:
        columns["packed3"] = dict(dtype=torch.uint8, layout="interleaved")
    with torch.cuda.stream(ctx.stream):
        b = ctx.encode(fmt, d_pcm, n)
        ctx.synchronize()
        out = ctx.decode(cookie, b["out"], b["offsets"], n)
        ctx.synchronize()
        assert torch.equal(out[0], d_pcm), "round trip differs"
        del d_pcm
        r["decode"] = rounds_ms(ctx, lambda: ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3]))
        fl = ctx.decode_float(cookie, b["out"], b["offsets"], n)
        fout = (fl[0], fl[1], fl[2])
        r["decode_float"] = rounds_ms(ctx, lambda: ctx.decode_float(cookie, b["out"], b["offsets"], n, out=fout))
        del fl, fout
        for name, kw in columns.items():
            got = ctx.decode_int(cookie, b["out"], b["offsets"], n, **kw)
            ctx.synchronize()
            if name == "packed3":
                assert torch.equal(got[0].view(-1), out[0]), "packed 3-byte decode_int differs from decode"
            else:
                assert torch.equal(got[0], composed(out[0], depth, 2, name)), name + " differs from decode + conversion"
            iout = (got[0], got[1], got[2])
            r[name] = rounds_ms(ctx, lambda: ctx.decode_int(cookie, b["out"], b["offsets"], n, out=iout, **kw))
            del got, iout
            if name != "packed3":
                def decode_convert():
                    ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3])
                    return composed(out[0], depth, 2, name)

                r["composed_" + name] = rounds_ms(ctx, decode_convert, reps=5, warm=2)
        # the float column once more behind the integer ones: what the run itself moves by
        fl = ctx.decode_float(cookie, b["out"], b["offsets"], n)
        fout = (fl[0], fl[1], fl[2])
        r["decode_float_again"] = rounds_ms(ctx, lambda: ctx.decode_float(cookie, b["out"], b["offsets"], n, out=fout))
        del fl, fout
    f, g, i = r["decode_float"], r["decode_float_again"], r["int32_planar"]
    own = i["spread_ms"][1] - i["spread_ms"][0]
    # the window of the float column measured in front of the integer columns, and of both float columns of the run
    first = [f["spread_ms"][0] - own, f["spread_ms"][1] + own]
    both = [min(f["spread_ms"][0], g["spread_ms"][0]) - own, max(f["spread_ms"][1], g["spread_ms"][1]) + own]
    # the composed route of the packed containers is decode itself: they are its bytes
    beats = {k: r[k]["ms"] < r["decode" if k == "packed3" else "composed_" + k]["ms"] for k in columns}
    r["bars"] = {"float_window_ms": first, "int32_planar_within_float_window": first[0] <= i["ms"] <= first[1],
                 "float_window_both_ms": both, "int32_planar_within_float_window_both": both[0] <= i["ms"] <= both[1],
                 "int32_planar_below_float_window": i["ms"] < first[0],
                 "beats_composed": beats,
                 "over_int32_planar": {k: r[k]["ms"] / i["ms"] for k in columns if k != "int32_planar"}}
    torch.cuda.empty_cache()
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    ap.add_argument("--depths", default="16,24")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(n), int(d)) for d in a.depths.split(",") for n in a.packets.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
