"""CPU: what alacconvert says when it refuses a command — usage errors, files it cannot take, --crc / --crc-check of files that
never reach the GPU — replayed against the recording in tests/golden/alacconvert_refusals.json (tests/make_cli_golden.py):
exit code, stdout and stderr, all three equal.  Every case returns before the first GPU call."""
import json
import os
import subprocess

import pytest

import make_cli_golden as g

with open(g.GOLDEN) as f:
    RECORDED = json.load(f)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    subprocess.check_call(["make", "-C", os.path.dirname(g.BIN), "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("cli")
    g.write_inputs(str(d))
    return str(d)


def test_the_recording_holds_every_case():
    assert [c[0] for c in RECORDED] == g.CASES
    assert len(g.USAGE) >= 40
    assert all(c[1] == 1 for c in RECORDED)  # every one is a refusal


@pytest.mark.parametrize("case", RECORDED, ids=[" ".join(c[0]) or "(none)" for c in RECORDED])
def test_refusal_is_the_recorded_one(workdir, case):
    before = sorted(os.listdir(workdir))
    assert g.run_case(case[0], workdir) == case
    assert sorted(os.listdir(workdir)) == before  # and nothing was written
