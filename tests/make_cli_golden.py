#!/usr/bin/env python3
"""Records what alacconvert says when it refuses a command: tests/golden/alacconvert_refusals.json, a list of
[argv, returncode, stdout, stderr].  Every case returns before the first GPU call, so the recording (and its replay,
tests/test_alacconvert_cli.py) needs no device.

Run against the binary whose behaviour is to be PINNED (the commit before a change to convert-utility/), never against the
code under test:   python tests/make_cli_golden.py

The commands run in a scratch directory that holds the files of write_inputs(), under relative names: the recorded text
carries no absolute path.
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import caf_oracle as co  # noqa: E402
from container_lib import music_like  # noqa: E402

BIN = os.path.join(ROOT, "convert-utility", "alacconvert")
GOLDEN = os.path.join(HERE, "golden", "alacconvert_refusals.json")

# options that neither --compare nor --crc takes
ALONE = [["--batch"], ["--lpc"], ["--verify"], ["--verify-source"], ["--segment-packets", "2"], ["--float-bits", "16"],
         ["--float-bits", "auto"]]

USAGE = [
    [], ["-h"], ["-x", "a", "b"],
    ["a"], ["a", "b", "c"], ["--batch", "a", "b", "c"], ["--batch"],
    ["--segment-packets", "0", "a", "b"], ["--devices", "0", "--batch", "a", "b"], ["--devices", "2", "a", "b"],
    ["--float-bits", "17", "a", "b"], ["--dither-seed", "zz", "a", "b"], ["a", "b", "--dither-seed"], ["--crc-check", ""],
    ["a", "b", "--devices"], ["a", "b", "--segment-packets"], ["a", "b", "--float-bits"], ["--crc-check"],
] + [["--compare"] + o + ["a", "b"] for o in ALONE] + [
    ["--compare", "--devices", "2", "--batch", "a", "b"], ["--compare", "a"], ["--compare", "a", "b", "c"],
    ["--crc"],
] + [["--crc"] + o + ["a.wav"] for o in ALONE] + [
    ["--crc", "--devices", "2", "--batch", "a.wav"], ["--crc", "--compare", "a.wav"], ["--crc", "--dither", "a.wav"],
    ["--crc-check", "list", "extra"], ["--crc", "--crc-check", "list", "x"], ["--crc-check", "list", "--lpc"],
    ["--dither", "a", "b"], ["--float-bits", "32", "--dither", "a", "b"], ["--float-bits", "auto", "--dither", "a", "b"],
    ["--verify-source", "a", "b"], ["--float-bits", "16", "--verify", "a", "b"],
    ["--float-bits", "16", "--float-bits", "auto", "--verify", "a", "b"],
]

FILES = [
    ["missing.wav", "o.caf"], ["junk.wav", "o.caf"], ["u8.wav", "o.caf"], ["ch9.wav", "o.caf"],
    ["--float-bits", "16", "good.wav", "o.caf"], ["--float-bits", "auto", "good.wav", "o.caf"],
    ["--float-bits", "16", "f64.wav", "o.caf"],
    ["--batch", "good.wav", "o1.caf", "missing.wav", "o2.caf"], ["--batch", "missing.wav", "o1.caf", "junk.wav", "o2.caf"],
    # an ALAC file the container parse refuses is named after every file was opened and sniffed
    ["nokuki.caf", "o.wav"], ["--batch", "nokuki.caf", "o1.wav", "missing.wav", "o2.caf"],
    ["--batch", "good.wav", "o1.caf", "nokuki.caf", "o2.wav", "u8.wav", "o3.caf"],
    ["--compare", "missing.caf", "good.wav"], ["--compare", "good.wav", "mono24.wav"], ["--compare", "junk.wav", "good.wav"],
    ["--compare", "nokuki.caf", "good.wav"], ["--compare", "nokuki.caf", "f64.wav"],
    ["--compare", "--dither", "nokuki.caf", "good.wav"],
]

CRC = [
    ["--crc", "missing.wav"], ["--crc", "f32.wav"], ["--crc", "junk.wav", "u8.wav", "ch9.wav", "nokuki.caf"],
    ["--crc-check", "missing.list"], ["--crc-check", "bad.list"],
]

CASES = USAGE + FILES + CRC


def retagged_float(wav):
    """a WAVE file written as format tag 1 with its tag set to 3 (IEEE float): 'RIFF' size 'WAVE' 'fmt ' size tag"""
    assert wav[12:16] == b"fmt "
    return wav[:20] + struct.pack("<H", 3) + wav[22:]


def write_inputs(d):
    """the files the cases name, into directory d (anything else a case names does not exist)"""
    files = {
        "good.wav": co.make_wav(music_like(4096 + 77, 2, 16, 1), 2, 44100, 16),
        "mono24.wav": co.make_wav(music_like(100, 1, 24, 2), 1, 48000, 24),
        "junk.wav": b"not a wave file at all",
        "u8.wav": co.make_wav(bytes(range(64)), 1, 8000, 8),
        "ch9.wav": co.make_wav(music_like(10, 9, 16, 3), 9, 44100, 16),
        "f32.wav": retagged_float(co.make_wav(struct.pack("<8f", *[i / 16.0 for i in range(8)]), 2, 44100, 32)),
        "f64.wav": retagged_float(co.make_wav(struct.pack("<8d", *[i / 16.0 for i in range(8)]), 1, 44100, 64)),
        # 'desc' says ALAC from a 16-bit source, and there is no magic cookie
        "nokuki.caf": b"caff\x00\x01\x00\x00" + b"desc" + struct.pack(">q", 32)
        + struct.pack(">d4sIIIII", 44100.0, b"alac", 1, 0, 4096, 2, 0) + b"data" + struct.pack(">q", 4) + b"\0\0\0\0",
        # a well-formed line for a file that is not there, single blanks, a CRC that is not hex, an empty line
        "bad.list": b"0123abcd  77  missing.wav\n0123abcd 77 good.wav\n0123abcg  77  good.wav\n\n",
    }
    assert len(files["junk.wav"]) == 22
    for name, data in files.items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)


def run_case(argv, cwd):
    p = subprocess.run([BIN] + argv, capture_output=True, text=True, timeout=60, cwd=cwd)
    return [argv, p.returncode, p.stdout, p.stderr]


def main():
    with tempfile.TemporaryDirectory() as d:
        write_inputs(d)
        before = sorted(os.listdir(d))
        out = [run_case(argv, d) for argv in CASES]
        assert sorted(os.listdir(d)) == before, "a refusal wrote a file"
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("%s: %d cases" % (os.path.relpath(GOLDEN, ROOT), len(out)))


if __name__ == "__main__":
    main()
