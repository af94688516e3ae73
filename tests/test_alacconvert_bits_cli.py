"""CPU: what alacconvert says when it refuses a command that names --bits — the options --bits does not go with, a depth it
does not take, inputs that are no integer PCM, --dither where nothing would be rounded — by exit code and key phrase, with
nothing written; and the --bits lines of the usage text appear exactly when the command line names --bits (the text without
them is pinned by tests/test_alacconvert_cli.py).  Every case returns before the first GPU call."""
import os
import subprocess

import pytest

import make_cli_golden as g


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.dirname(g.BIN), "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("bits_cli")
    g.write_inputs(str(d))
    return str(d)


def run(argv, workdir):
    before = sorted(os.listdir(workdir))
    _, rc, out, err = g.run_case(argv, workdir)
    assert sorted(os.listdir(workdir)) == before, argv  # nothing was written
    return rc, out, err


# (argv, the phrase of the one line on stderr)
ONE_LINE = [
    (["--bits", "16", "--float-bits", "16", "good.wav", "o.caf"], "not with --float-bits"),
    (["--float-bits", "auto", "--bits", "auto", "good.wav", "o.caf"], "not with --float-bits"),
    (["--bits", "16", "--compare", "nokuki.caf", "good.wav"], "not with --compare"),
    (["--crc", "--bits", "24", "good.wav"], "not with --crc"),
    (["--bits", "auto", "--crc-check", "bad.list"], "not with --crc-check"),
    (["--bits", "17", "good.wav", "o.caf"], "--bits takes 16, 20, 24, 32 or auto"),
    (["--bits", "0", "good.wav", "o.caf"], "--bits takes 16, 20, 24, 32 or auto"),
    (["--bits", "8", "--batch", "good.wav", "o.caf"], "--bits takes 16, 20, 24, 32 or auto"),
    (["--bits", "Auto", "good.wav", "o.caf"], "--bits takes 16, 20, 24, 32 or auto"),
]


@pytest.mark.parametrize("argv,phrase", ONE_LINE, ids=[" ".join(a) for a, _ in ONE_LINE])
def test_refused_with_one_line(workdir, argv, phrase):
    rc, out, err = run(argv, workdir)
    assert rc == 1 and out == ""
    assert err.count("\n") == 1 and phrase in err, err


# (argv, the phrase, the file named)
FILES = [
    (["--bits", "16", "nokuki.caf", "o.wav"], "--bits takes integer PCM input, not float PCM or ALAC", "nokuki.caf"),
    (["--bits", "auto", "f32.wav", "o.caf"], "--bits takes integer PCM input, not float PCM or ALAC", "f32.wav"),
    (["--bits", "24", "--batch", "good.wav", "o1.caf", "f32.wav", "o2.caf"], "--bits takes integer PCM input", "f32.wav"),
    (["--bits", "16", "--dither", "good.wav", "o.caf"], "would round nothing", "good.wav"),
    (["--bits", "24", "--dither", "--batch", "good.wav", "o1.caf", "mono24.wav", "o2.caf"], "would round nothing", "good.wav"),
    (["--bits", "24", "--dither", "--dither-seed", "7", "mono24.wav", "o.caf"], "would round nothing", "mono24.wav"),
    (["--bits", "16", "u8.wav", "o.caf"], "unsupported type", "u8.wav"),
    (["--bits", "16", "missing.wav", "o.caf"], "Cannot open file", "missing.wav"),
]


@pytest.mark.parametrize("argv,phrase,name", FILES, ids=[" ".join(a) for a, _, _ in FILES])
def test_file_refused_by_name(workdir, argv, phrase, name):
    rc, out, err = run(argv, workdir)
    assert rc == 1
    assert err.count("\n") == 1 and phrase in err and name in err, err


BITS_LINES = ("alacconvert --bits N [--dither [--dither-seed S]]", "alacconvert --bits auto")
# the usage text, with the --bits lines behind it
WITH = [["--bits"], ["--bits", "16"], ["--bits", "16", "a"], ["--bits", "auto", "a", "b", "c"], ["--bits", "16", "-h"],
        ["--bits", "16", "--devices", "2", "a", "b"], ["--bits", "auto", "--dither", "good.wav", "o.caf"],
        ["--bits", "32", "--dither", "good.wav", "o.caf"]]
# ... and without them
WITHOUT = [[], ["-h"], ["a"], ["--float-bits", "17", "a", "b"], ["--dither", "a", "b"], ["--float-bits", "auto", "--dither", "a", "b"]]


def usage_text(workdir):
    rc, out, err = run(["-h"], workdir)
    assert rc == 1 and out.startswith("Usage:\n") and err == ""
    return out


@pytest.mark.parametrize("argv", WITH, ids=[" ".join(a) for a in WITH])
def test_usage_with_the_bits_lines(workdir, argv):
    rc, out, err = run(argv, workdir)
    usage = usage_text(workdir)
    assert rc == 1 and out.startswith(usage) and len(out) > len(usage)
    tail = out[len(usage):]
    assert all(line in tail for line in BITS_LINES) and not any(line in usage for line in BITS_LINES)
    if "--dither" in argv:
        assert err == " --dither needs --bits 16, 20 or 24\n"


@pytest.mark.parametrize("argv", WITHOUT, ids=[" ".join(a) or "(none)" for a in WITHOUT])
def test_usage_without_the_bits_lines(workdir, argv):
    rc, out, err = run(argv, workdir)
    assert rc == 1 and out == usage_text(workdir)
    assert "--bits" not in out and "--bits" not in err
    if argv[:1] == ["--dither"]:
        assert err == " --dither needs --float-bits 16, 20 or 24\n"  # today's message
