"""CPU: the pure pieces of alacconvert (convert-utility/plan.h: the command line, the packet cut, the deal of files to workers,
a line of a --crc list) against literal expectations, in a stand-alone program of its own built with the address and
undefined-behaviour sanitizers (tests/cpp/convert_plan.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_the_pure_pieces_of_alacconvert():
    subprocess.check_call(["make", "-C", CPP, "convert_plan"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(CPP, "convert_plan")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.splitlines()[-1] == "ok"
