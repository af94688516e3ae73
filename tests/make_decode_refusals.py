#!/usr/bin/env python3
"""Records what the decode family says when it refuses a call: tests/golden/decode_refusals.json, a list of
{"rig", "entry", "case", "status", "error", "touched"} in call order.

The family is alac_hip_decode, _decode_float, _decode_int, _verify and _verify_float, each with its host form.  Every entry
point gets its accepted base call and then one call per refusal its source has: each null pointer in turn, misaligned and
short buffers, bad cookies, bad strides, bad descriptors.  "status" is the return value, "error" the text of
alac_hip_last_error behind a refusal, "touched" the names of the output buffers (filled with a sentinel byte in front of
every call) in which a byte changed.

Run against the library whose behaviour is to be PINNED (the commit before a change to the decode family's plumbing), never
against the code under test, on a machine with a GPU:

    ALAC_HIP_LIB=/path/to/that/libalac_hip.so python tests/make_decode_refusals.py

tests/test_gpu_decode_refusals.py replays the list through record() and compares.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

GOLDEN = os.path.join(HERE, "golden", "decode_refusals.json")
SENT = 0xC3
FRAME, PACKETS = 256, 2
T = FRAME * PACKETS

# the parameters of the ten entry points behind the context, in the order of include/alac_hip.h
PARAMS = {
    "decode": "cookie cookie_size stream offsets np ws wsb pcm ns st",
    "decode_float": "cookie cookie_size stream offsets np ws wsb pcm cs ns st",
    "decode_int": "cookie cookie_size stream offsets np ws wsb pcm dst ns st",
    "verify": "cookie cookie_size stream offsets np expected nse ws vwsb fm st bad",
    "verify_float": "cookie cookie_size stream offsets np source cs fs nse dither origin ws vwsb fm st bad",
    "decode_host": "cookie cookie_size h_stream h_sizes np h_pcm h_ns h_st",
    "decode_float_host": "cookie cookie_size h_stream h_sizes np h_pcm cs h_ns h_st",
    "decode_int_host": "cookie cookie_size h_stream h_sizes np h_pcm dst h_ns h_st",
    "verify_host": "cookie cookie_size h_stream h_sizes np h_expected h_nse h_fm h_st",
    "verify_float_host": "cookie cookie_size h_stream h_sizes np h_source cs fs h_nse dither h_origin h_fm h_st",
}
SCALARS = {"cookie_size", "np", "wsb", "vwsb", "cs", "fs"}
# the refusals that come behind a call's first launch: alac_hip_verify has initialised its two outputs by the time the decode
# pass looks at the cookie's AG parameters
LATE = {("verify", "cookie kb 0"): ["fm", "bad"], ("verify_float", "cookie kb 0"): ["fm", "bad"]}


class Rig:
    """one stream of PACKETS packets, its inputs on both sides, and sentinel-filled outputs on both sides"""
    params = PARAMS  # entry point -> its parameter names (tests/make_encode_refusals.py: the encode family's)

    def __init__(self, ctx, name, depth, channels):
        import torch
        import alac_amd
        from test_gpu_verify import encode_case
        self.ctx, self.name, self.torch = ctx, name, torch
        self.IntSource, self.Dither = alac_amd.capi.IntSource, alac_amd.capi.Dither
        c = encode_case(ctx, depth, channels, T, seed=21, frame_size=FRAME)
        assert c.n == PACKETS
        self.depth, self.channels, fmt = depth, channels, c.fmt
        bps = alac_amd.capi.BPS[depth]
        # the float source of the stream: its own PCM, scaled (planar rows of T floats)
        raw = c.expected.reshape(T, channels, bps).astype(np.int32)
        val = sum(raw[:, :, k] << (8 * k) for k in range(bps))
        val = (val << (32 - 8 * bps)) >> (32 - 8 * bps) >> (8 * bps - depth)
        source = np.ascontiguousarray((val.T / float(1 << (depth - 1))).astype(np.float32))
        sizes = c.sizes.astype(np.uint32)
        offsets = np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int64)
        origin = (np.arange(PACKETS) * FRAME).astype(np.uint64)
        counts = c.counts.astype(np.uint32)
        cookies = {"cookie": c.cookie.copy(), "short": c.cookie[:10].copy(), "kb0": c.cookie.copy(), "depth17": c.cookie.copy()}
        cookies["kb0"][8] = 0
        cookies["depth17"][5] = 17
        self.cookies = cookies
        self.host_in = {"h_stream": c.stream, "h_sizes": sizes, "h_expected": c.expected, "h_source": source, "h_nse": counts,
                        "h_origin": origin}
        dev = lambda a: torch.from_numpy(a).cuda()
        self.dev_in = {"stream": dev(c.stream), "offsets": dev(offsets), "expected": dev(c.expected), "source": dev(source),
                       "nse": dev(counts.view(np.int32)), "origin": dev(origin.view(np.int64))}
        lib = ctx.lib
        self.wsb = int(lib.alac_hip_decode_workspace_bytes_stream(C.byref(fmt), PACKETS, c.stream.size))
        self.vwsb = int(lib.alac_hip_verify_workspace_bytes_stream(C.byref(fmt), PACKETS, c.stream.size))
        self.ws = torch.empty(self.vwsb + 256, dtype=torch.uint8, device="cuda")
        # outputs: name -> (offset, bytes) in one buffer per side; pcm holds any mode's PCM (4-byte containers) and a tail
        self.slots, at = {}, 0
        for k, n in (("pcm", channels * T * 4 + 64), ("ns", PACKETS * 4), ("st", PACKETS * 4), ("fm", PACKETS * 4), ("bad", 4)):
            self.slots[k] = (at, n)
            at += (n + 255) // 256 * 256
        self.d_out = torch.empty(at, dtype=torch.uint8, device="cuda")
        self.h_out = np.empty(at, np.uint8)
        self.refill()

    def refill(self):
        self.d_out.fill_(SENT)
        self.h_out[:] = SENT
        self.torch.cuda.synchronize()

    def touched(self):
        """names of the outputs, device then host, in which a byte is no longer the sentinel"""
        d = self.d_out.cpu().numpy()
        names = [k for k, (at, n) in self.slots.items() if (d[at:at + n] != SENT).any()]
        names += ["h_" + k for k, (at, n) in self.slots.items() if (self.h_out[at:at + n] != SENT).any()]
        return names

    def base(self):
        """every parameter's value in the accepted call: addresses as int, scalars as int, structs as ctypes structures"""
        b = {"cookie": self.cookies["cookie"].ctypes.data, "cookie_size": self.cookies["cookie"].size, "np": PACKETS,
             "ws": self.ws.data_ptr(), "wsb": self.wsb, "vwsb": self.vwsb, "cs": T, "fs": 1,
             "dst": self.IntSource(4, 32, 1, 0, T, 1), "dither": self.Dither(1, 0, 5)}
        b.update({k: v.data_ptr() for k, v in self.dev_in.items()})
        b.update({k: v.ctypes.data for k, v in self.host_in.items()})
        b.update({k: self.d_out.data_ptr() + at for k, (at, n) in self.slots.items()})
        b.update({"h_" + k: self.h_out.ctypes.data + at for k, (at, n) in self.slots.items()})
        return b

    def call(self, entry, over):
        b = self.base()
        b.update(over)
        args = [C.byref(b[p]) if isinstance(b[p], C.Structure) else b[p] for p in self.params[entry].split()]
        h = None if over.get("ctx", 1) is None else self.ctx.h
        rc = getattr(self.ctx.lib, "alac_hip_" + entry)(h, *args)
        self.ctx.lib.alac_hip_synchronize(self.ctx.h)
        self.torch.cuda.synchronize()
        text = self.ctx.lib.alac_hip_last_error(self.ctx.h).decode() if rc < 0 and h is not None else ""
        touched = self.touched()
        if touched:
            self.refill()
        return rc, text, touched

    # ---- the cases of an entry point: (label, overrides of the base call) ----
    def cases(self, entry):
        b, host = self.base(), entry.endswith("_host")
        names = PARAMS[entry].split()
        out = [("base", {}), ("null context", {"ctx": None})]
        out += [("null " + p, {p: None}) for p in names if p not in SCALARS]
        out += [("cookie truncated", {"cookie": self.cookies["short"].ctypes.data, "cookie_size": 10}),
                ("cookie kb 0", {"cookie": self.cookies["kb0"].ctypes.data}),
                ("cookie depth 17", {"cookie": self.cookies["depth17"].ctypes.data}),
                ("no packets", {"np": 0})]
        if not host:
            w = "vwsb" if "vwsb" in names else "wsb"
            out += [("workspace misaligned", {"ws": b["ws"] + 1}), ("workspace one byte short", {w: b[w] - 1})]
        if entry == "decode":
            out += [("pcm misaligned", {"pcm": b["pcm"] + 1})]
        if entry.startswith("decode_float"):
            if not host:
                out += [("out misaligned", {"pcm": b["pcm"] + 2})]
            out += [("channel_stride one below", {"cs": T - 1}), ("channel_stride overflows", {"cs": 1 << 62}),
                    ("channel_stride with a gap", {"cs": T + 3})]
        if entry.startswith("decode_int"):
            p = "h_pcm" if host else "pcm"
            dst = lambda cb=4, bits=32, lj=1, res=0, cs=T, fs=1: {"dst": self.IntSource(cb, bits, lj, res, cs, fs)}
            out += [("container_bytes 5", dst(cb=5)), ("container_bytes 1", dst(cb=1)), ("bits 23", dst(bits=23)),
                    ("bits above the container", dst(cb=3, bits=32)), ("reserved 1", dst(res=1)), ("left_justified 2", dst(lj=2)),
                    ("out not aligned to its container", {p: b[p] + 2}), ("frame_stride 0", dst(fs=0)),
                    ("channel_stride 0", dst(cs=0, fs=2)), ("largest index overflows", dst(cs=1 << 62)),
                    ("bits below the depth", dst(bits=16, lj=0)), ("bits 20 right-justified", dst(bits=20, lj=0)),
                    ("samples share a container", dst(cs=T - 1)), ("samples share a container, strided", dst(cs=3 * T - 1, fs=3)),
                    ("interleaved", dst(cs=1, fs=self.channels)), ("int16 at an odd address", {p: b[p] + 1, **dst(cb=2, bits=16)}),
                    ("packed 24 at an odd address", {p: b[p] + 1, **dst(cb=3, bits=24)})]
        if entry.startswith("verify"):
            if not host:
                out += [("no packets, null bad", {"np": 0, "bad": None})]
                if entry == "verify":
                    out += [("expected misaligned", {"expected": b["expected"] + 1})]
            else:
                out += [("2^31 packets", {"np": 1 << 31})]
        if entry.startswith("verify_float"):
            s, o = ("h_source", "h_origin") if host else ("source", "origin")
            out += [("dither mode 2", {"dither": self.Dither(2, 0, 5)}), ("dither reserved 1", {"dither": self.Dither(1, 1, 5)}),
                    ("dither none", {"dither": self.Dither(0, 0, 5)}), ("origin misaligned", {o: b[o] + 4}),
                    ("origin misaligned, dither none", {o: b[o] + 4, "dither": self.Dither(0, 0, 5)}),
                    ("no packets, dither mode 2", {"np": 0, "dither": self.Dither(2, 0, 5)}),
                    ("source misaligned", {s: b[s] + 2}), ("frame_stride 0", {"fs": 0}), ("channel_stride 0", {"cs": 0, "fs": 2}),
                    ("largest index overflows", {"cs": 1 << 62})]
        return out


def record(ctx):
    """every case of every entry point on both rigs, in order -> the list the golden file holds"""
    out = []
    # stereo at 16 bits; six channels (the element rounds and their host wait) at 24 bits (a depth that bits can lie below)
    for name, depth, channels in (("stereo16", 16, 2), ("six24", 24, 6)):
        rig = Rig(ctx, name, depth, channels)
        for entry in PARAMS:
            for label, over in rig.cases(entry):
                rc, text, touched = rig.call(entry, over)
                out.append({"rig": name, "entry": entry, "case": label, "status": rc, "error": text, "touched": touched})
    return out


def main():
    import alac_amd
    out = record(alac_amd.Context(0))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("%s: %d calls, %d refused, library %s" % (os.path.relpath(GOLDEN, ROOT), len(out), sum(e["status"] < 0 for e in out),
                                                    alac_amd.capi.LIB_PATH))


if __name__ == "__main__":
    main()
