#!/usr/bin/env python3
"""Records what the encode family says when it refuses a call: tests/golden/encode_refusals.json, a list of
{"rig", "entry", "case", "status", "error", "touched"} in call order (one call per line).

The family is alac_hip_encode, _encode_segmented, _encode_float, _encode_float_dither, _encode_int and _pcm_requantize, and
the host forms _encode_host, _encode_host_segments, _encode_float_host, _encode_float_dither_host, _encode_int_host and
_pcm_requantize_host.  Every entry point gets its accepted base call and then one call per refusal its source has: each
pointer null in turn, misaligned and short buffers, bad segment counts and tables, bad strides, bad alac_hip_int_source and
alac_hip_dither structs, no packets; calls with two faults pin the order of the checks.  The fields and the sentinel-filled
outputs are those of tests/make_decode_refusals.py, whose Rig makes the calls.

No case may run a kernel over a buffer it breaks: a case is either refused or an accepted call over valid buffers (a nullable
pointer left out, a stride the format does not use, a table LPC mode ignores).  That is why the 3-channel rig leaves out a
misaligned `out` and `pcm` (that form checks the alignment of its workspace only), why the host float forms leave out a
misaligned `h_in`, and why the one place where the largest-index test of a float source is `>` and not `>=`
(float_stride_refusal) is pinned through the host forms alone, whose span test in front of it is `>=`.

Run against the library whose behaviour is to be PINNED (the commit before a change to the encode family's plumbing), never
against the code under test, on a machine with a GPU:

    ALAC_HIP_LIB=/path/to/that/libalac_hip.so python tests/make_encode_refusals.py

tests/test_gpu_encode_refusals.py replays the list through record() and compares.
"""
import ctypes as C
import json
import os

import numpy as np

import make_decode_refusals as dec
from make_decode_refusals import HERE, ROOT

GOLDEN = os.path.join(HERE, "golden", "encode_refusals.json")
FRAME, PACKETS = 256, 2
T = FRAME * PACKETS

_DEV = "seg nseg maxseg state state_in ws fwsb out cap sizes offs"
_HOST = "h_seg nseg h_state state_in h_out cap h_sizes h_total"
# the parameters of the twelve entry points behind the context, in the order of include/alac_hip.h
PARAMS = {
    "encode": "fmt pcm ns np seg nseg state state_in ws wsb out cap sizes offs",
    "encode_segmented": "fmt pcm ns np seg nseg maxseg state state_in ws wsb out cap sizes offs",
    "encode_float": "fmt fin cs fs ns np " + _DEV + " clipped",
    "encode_float_dither": "fmt fin cs fs ns np " + _DEV + " clipped dither origin",
    "encode_int": "fmt iin src ns np " + _DEV + " clipped dither origin",
    "pcm_requantize": "fmt iin src ns np pcmout pcmcap clipped dither origin",
    "encode_host": "fmt h_pcm samples segpk h_state state_in h_out cap h_sizes h_total",
    "encode_host_segments": "fmt h_pcm h_ns np " + _HOST,
    "encode_float_host": "fmt h_fin cs fs h_ns np " + _HOST + " h_clipped",
    "encode_float_dither_host": "fmt h_fin cs fs h_ns np " + _HOST + " h_clipped dither h_origin",
    "encode_int_host": "fmt h_iin src h_ns np " + _HOST + " h_clipped dither h_origin",
    "pcm_requantize_host": "fmt h_iin src h_ns np h_pcmout pcmcap h_clipped dither h_origin",
}
SCALARS = {"np", "nseg", "maxseg", "state_in", "wsb", "fwsb", "cap", "pcmcap", "cs", "fs", "samples", "segpk"}
# what a refused call may have written: a host form zeroes *out_total_bytes in front of its checks
EARLY = ["h_total"]
# ... and the one refusal behind a call's first launch: a 3..8-channel call reads a table without a bound back per element
# group, behind the conversion, whose launcher has zeroed the clip counters
LATE = {("three16", "encode_float_dither", "segment table descending, no bound"): ["clipped"]}
# alac_hip_encode_workspace_bytes always counts the LPC table (64 bytes per packet and channel of two, in 256-byte blocks), which
# a call without option "lpc" does not ask for
LPC_TABLE = (PACKETS * 2 * 64 + 255) // 256 * 256
# entry points that only pass a constant on to another one's code: they get the base call, the nulls and little else
TWINS = {"encode": "encode_segmented", "encode_float": "encode_float_dither", "encode_float_host": "encode_float_dither_host"}
SPARE = 8  # entries of a segment table and segments of a state buffer: a count above num_packets still reads inside them


class Rig(dec.Rig):
    """one batch of PACKETS packets as packed PCM, planar float32 and planar left-justified int32, on both sides, and
    sentinel-filled outputs on both sides; opts: the options the rig's calls run under"""
    params = PARAMS

    def __init__(self, ctx, name, depth, channels, opts=()):
        import torch
        import alac_amd
        self.ctx, self.name, self.torch, self.opts = ctx, name, torch, dict(opts)
        self.Format, self.IntSource, self.Dither = alac_amd.capi.Format, alac_amd.capi.IntSource, alac_amd.capi.Dither
        self.depth, self.channels = depth, channels
        self.fmt = alac_amd.make_format(FRAME, depth, channels, 44100)
        bps = alac_amd.capi.BPS[depth]
        rng = np.random.default_rng(31)
        val = rng.integers(-(1 << (depth - 2)), 1 << (depth - 2), size=(channels, T)).astype(np.int32)
        wide = np.ascontiguousarray(val << (32 - depth))                                     # planar, left-justified int32
        packed = (np.ascontiguousarray(val.T).astype("<i4") << (8 * bps - depth)).view(np.uint8).reshape(T, channels, 4)[:, :, :bps]
        seg = np.array([0, 1, 2] + [2] * (SPARE - 3), np.uint32)
        self.tables = {"seg": seg, "descending": np.array([0, 3, 2] + [2] * (SPARE - 3), np.uint32)}
        self.host_in = {"h_pcm": np.ascontiguousarray(packed).reshape(-1), "h_fin": (val / float(1 << (depth - 1))).astype(np.float32),
                        "h_iin": wide, "h_ns": np.full(PACKETS, FRAME, np.uint32), "h_seg": seg,
                        "h_origin": (np.arange(PACKETS) * FRAME).astype(np.uint64)}
        self.h_descending = self.tables["descending"]
        self.h_short = np.array([FRAME, 1], np.uint32)  # frame counts with a short last packet
        dev = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else
                                         a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
        self.dev_in = {k[2:]: dev(v) for k, v in self.host_in.items()}
        self.d_descending = dev(self.tables["descending"])
        lib, f = ctx.lib, C.byref(self.fmt)
        self.wsb = int(lib.alac_hip_encode_workspace_bytes(f, PACKETS, PACKETS))
        self.fwsb = int(lib.alac_hip_encode_float_workspace_bytes(f, PACKETS, PACKETS))
        self.stage = self.fwsb - (self.wsb + 255) // 256 * 256  # the staged PCM at the end of a float / int workspace
        self.cap = int(lib.alac_hip_encode_max_output_bytes(f, PACKETS))
        self.pcmcap = T * channels * bps
        self.ws = torch.empty(self.fwsb + 256, dtype=torch.uint8, device="cuda")
        state = SPARE * int(lib.alac_hip_state_int16(f)) * 2
        self.slots, at = {}, 0
        for k, n in (("out", self.cap + 64), ("sizes", PACKETS * 4), ("offs", (PACKETS + 1) * 8), ("state", state),
                     ("clipped", PACKETS * 4), ("pcmout", self.pcmcap + 64), ("total", 8)):
            self.slots[k] = (at, n)
            at += (n + 255) // 256 * 256
        self.d_out = torch.empty(at, dtype=torch.uint8, device="cuda")
        self.h_out = np.empty(at, np.uint8)
        self.refill()

    def base(self):
        b = {"fmt": self.fmt, "np": PACKETS, "nseg": PACKETS, "maxseg": 1, "state_in": 0, "ws": self.ws.data_ptr(),
             "wsb": self.wsb, "fwsb": self.fwsb, "cap": self.cap, "pcmcap": self.pcmcap, "cs": T, "fs": 1, "samples": T, "segpk": 1,
             "src": self.IntSource(4, 32, 1, 0, T, 1), "dither": self.Dither(1, 0, 5)}
        b.update({k: v.data_ptr() for k, v in self.dev_in.items()})
        b.update({k: v.ctypes.data for k, v in self.host_in.items()})
        b.update({k: self.d_out.data_ptr() + at for k, (at, n) in self.slots.items()})
        b.update({"h_" + k: self.h_out.ctypes.data + at for k, (at, n) in self.slots.items()})
        b["h_total"] = C.cast(b["h_total"], C.POINTER(C.c_uint64))
        return b

    def call(self, entry, over):
        """`over` may carry "opt": options set for this one call"""
        over = dict(over)
        with self.ctx.options(**over.pop("opt", {})):
            return super().call(entry, over)

    # ---- the cases of an entry point: (label, overrides of the base call) ----
    def source_cases(self, entry, b, host, every):
        """what a float or integer source and its dither can be refused for; every: each check of a struct, otherwise one
        case per place that calls the checks"""
        D, out = self.Dither, []
        if "float" in entry:
            p = "h_fin" if host else "fin"
            out += [("frame_stride 0", {"fs": 0}), ("channel_stride 0", {"cs": 0}), ("channel_stride overflows", {"cs": 1 << 62}),
                    ("frame_stride overflows", {"fs": 1 << 62})]
            if host:
                # the span test (>=, "h_in") stands in front of the stride test (>, "d_in"): the first refuses the largest index
                # the second lets pass; the second alone refuses whole packets behind a short last one
                near = (1 << 62) - 1 - (T - 1)
                out += [("largest index UINT64_MAX / 4", {"cs": near}), ("frame_stride 0, channel_stride overflows", {"fs": 0, "cs": 1 << 62}),
                        ("short last packet, whole packets overflow", {"cs": near + 200, "h_ns": self.h_short.ctypes.data})]
            else:
                out += [("d_in misaligned", {p: b[p] + 2})]
        else:
            p = "h_iin" if host else "iin"
            src = lambda cb=4, bits=32, lj=1, res=0, cs=T, fs=1: {"src": self.IntSource(cb, bits, lj, res, cs, fs)}
            out += [("container_bytes 5", src(cb=5)), ("in not aligned to its container", {p: b[p] + 2}),
                    ("channel_stride overflows", src(cs=1 << 62)), ("dither at the source's depth", src(bits=self.depth, lj=0)),
                    ("null in, bad dither", {p: None, "dither": D(2, 0, 5)})]
            if every:
                out += [("container_bytes 1", src(cb=1)), ("bits 23", src(bits=23)), ("bits above the container", src(cb=3, bits=32)),
                        ("reserved 1", src(res=1)), ("left_justified 2", src(lj=2)), ("frame_stride 0", src(fs=0)),
                        ("channel_stride 0", src(cs=0)), ("frame_stride overflows", src(fs=1 << 62))]
        if "dither" in self.params[entry]:
            o = "h_origin" if host else "origin"
            wide = self.Format(FRAME, 32, self.channels, 44100)
            out += [("dither mode 2", {"dither": D(2, 0, 5)}), ("dither at 32 bits", {"fmt": wide}), ("origin misaligned", {o: b[o] + 4}),
                    ("no packets, dither mode 2", {"np": 0, "dither": D(2, 0, 5)}), ("dither mode 2, null in", {p: None, "dither": D(2, 0, 5)})]
            if every:
                out += [("dither reserved 1", {"dither": D(1, 1, 5)}), ("dither none", {"dither": D(0, 0, 5)}),
                        ("dither none at 32 bits, no packets", {"fmt": wide, "dither": D(0, 0, 5), "np": 0}),
                        ("origin misaligned, dither none", {o: b[o] + 4, "dither": D(0, 0, 5)})]
        return out

    def cases(self, entry, full=True):
        """full: every case; otherwise the ones whose outcome depends on the rig's format or options"""
        b, host = self.base(), entry.endswith("_host") or entry == "encode_host_segments"
        names = self.params[entry].split()
        staged, requant = "fwsb" in names, entry.startswith("pcm_requantize")
        mc, lpc, mono = self.channels > 2, bool(self.opts.get("lpc")), self.channels == 1
        twin = entry in TWINS
        out = [("base", {})]
        if full:
            bad = {"fmt": self.Format(FRAME, 17, self.channels, 44100)}
            out += [("null context", {"ctx": None})]
            out += [("null " + p, {p: None}) for p in names if p not in SCALARS and (not twin or p == "fmt")]
            out += [("bad format", bad), ("bad format, null buffers", {**bad, **{p: None for p in names if p not in SCALARS | {"fmt"}}})]
            out += [("no packets", {"samples": 0} if entry == "encode_host" else {"np": 0})]
        if any(n in names for n in ("fin", "h_fin", "iin", "h_iin")):
            if full and not twin:
                out += self.source_cases(entry, b, host, entry in ("encode_float_dither", "encode_int"))
            elif full:
                out += [("frame_stride 0", {"fs": 0}), ("channel_stride overflows", {"cs": 1 << 62})]
            elif mono and not twin:  # a stride no channel uses is not looked at; 24 bits: another depth below the source's
                keep = ("channel_stride 0", "channel_stride overflows", "dither at the source's depth")
                out += [c for c in self.source_cases(entry, b, host, True) if c[0] in keep]
        if requant:
            p = "h_pcmout" if host else "pcmout"
            if full:
                out += [("pcm_capacity one byte short", {"pcmcap": b["pcmcap"] - 1})]
                out += [] if host else [("pcm out misaligned", {p: b[p] + 8})]
            return out
        if entry == "encode_host":
            if full:
                out += [("too many packets", {"samples": FRAME << 31}), ("one chained segment", {"segpk": 0}),
                        ("host output too small", {"cap": 16})]
            return out
        if mono or (twin and entry != "encode"):
            return out
        if not full and "iin" in "".join(names):  # the integer forms share the float forms' path behind the source's checks
            return out + ([] if host else [("workspace below the stage, null in", {"fwsb": self.stage - 1, "iin": None})])
        w = "fwsb" if staged else "wsb"
        s = "h_seg" if host else "seg"
        desc = (self.h_descending.ctypes.data if host else self.d_descending.data_ptr())
        short = b[w] - 1 - (0 if mc or lpc else LPC_TABLE)  # one byte below what the call asks for
        both = {"lpc": 1, "fast_mode": 1}
        if host:
            # the segment count and table (the host forms check the table in LPC mode too, which then ignores it)
            out += [("num_segments above num_packets", {"nseg": PACKETS + 1})]
            if full:
                out += [("num_segments 0", {"nseg": 0}), ("segment table descending", {s: desc}),
                        ("segment table ends below num_packets", {"nseg": 1}), ("host output too small", {"cap": 16})]
            if full or lpc:
                out += [("lpc and fast_mode", {"opt": both})]
            if mc:
                out += [("lpc", {"opt": {"lpc": 1}})]
            return out
        nobound = {} if "maxseg" not in names else {"maxseg": 0}
        out += [("segment table descending, no bound", {s: desc, **nobound})]
        if entry == "encode":
            if mc:
                out += [("too many packets", {"np": 1 << 29, "nseg": 1})]
            return out + ([("lpc and fast_mode, no packets", {"opt": both, "np": 0})] if full else [])
        # the segment count (LPC mode ignores it with the table)
        out += [("num_segments 0", {"nseg": 0}), ("num_segments above num_packets", {"nseg": PACKETS + 1})]
        if full:
            out += [("no bound", nobound)]
        # the caller's buffers
        out += [("workspace misaligned", {"ws": b["ws"] + 1}), ("workspace one byte short", {w: short})]
        if full or mc:
            out += [("output capacity one byte short", {"cap": b["cap"] - 1})]
        if full:
            out += [("out misaligned", {"out": b["out"] + 1})]
            out += [] if staged else [("pcm misaligned", {"pcm": b["pcm"] + 8})]
        if staged and (full or mc):
            p = "fin" if "fin" in names else "iin"
            out += [("workspace below the stage", {w: self.stage - 1}), ("workspace below the stage, null out", {w: self.stage - 1, "out": None}),
                    ("workspace below the stage, null in", {w: self.stage - 1, p: None}),
                    ("workspace one byte short, null in", {w: short, p: None})]
        elif full:
            out += [("workspace one byte short, null out", {w: short, "out": None}), ("num_segments 0, null out", {"nseg": 0, "out": None})]
        # options: LPC with fast_mode, with 3..8 channels, above 16 384 samples a packet; checked in front of num_packets = 0
        if full or lpc:
            at, above = self.Format(8192, self.depth, 2, 44100), self.Format(8193, self.depth, 2, 44100)
            out += [("lpc and fast_mode", {"opt": both}), ("lpc and fast_mode, no packets", {"opt": both, "np": 0}),
                    ("lpc, 8193 frames, no packets", {"opt": {"lpc": 1}, "fmt": above, "np": 0}),
                    ("lpc, 8192 frames, no packets", {"opt": {"lpc": 1}, "fmt": at, "np": 0})]
        if mc:
            out += [("lpc", {"opt": {"lpc": 1}}), ("lpc, no packets", {"opt": {"lpc": 1}, "np": 0})]
        return out


# rig, depth, channels, options, every case (or only those that depend on the rig)
RIGS = (("stereo16", 16, 2, {}, True), ("mono24", 24, 1, {}, False), ("three16", 16, 3, {}, False),
        ("stereo16 lpc", 16, 2, {"lpc": 1}, False))


def record(ctx):
    """every case of every entry point on every rig, in order -> the list the golden file holds"""
    out = []
    for name, depth, channels, opts, full in RIGS:
        rig = Rig(ctx, name, depth, channels, opts)
        with ctx.options(**opts):
            for entry in PARAMS:
                for label, over in rig.cases(entry, full):
                    rc, text, touched = rig.call(entry, over)
                    out.append({"rig": name, "entry": entry, "case": label, "status": rc, "error": text, "touched": touched})
    return out


def main():
    import alac_amd
    out = record(alac_amd.Context(0))
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(e, separators=(",", ":")) for e in out) + "\n]\n")
    print("%s: %d calls, %d refused, library %s" % (os.path.relpath(GOLDEN, ROOT), len(out), sum(e["status"] < 0 for e in out),
                                                    alac_amd.capi.LIB_PATH))


if __name__ == "__main__":
    main()
