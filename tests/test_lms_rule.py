"""CPU: the threshold form of the predictor's coefficient update (lms_adapt_thresholds, alac_amd/csrc/alac_lms.hpp: the one
spelling of the decoder's one-lane steps; the two-lane lms4_step_dec and the encoder's lms_step keep their own) against the
early-exit walk of the oracle's unpc_block, state by state, in a stand-alone program of its own built with the address and
undefined-behaviour sanitizers (tests/cpp/lms_rule.cpp holds the case table)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_the_threshold_form_is_the_oracles_walk():
    subprocess.check_call(["make", "-C", CPP, "lms_rule"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(CPP, "lms_rule")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.splitlines()[-1] == "ok"
