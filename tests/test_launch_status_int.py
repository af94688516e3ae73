"""launch_pcm_requantize as a stand-alone program (tests/cpp/launch_status_int.hip: alac_pcm_in.hip compiled in, the host
side under the address and undefined-behaviour sanitizers): what the launcher refuses comes back as hipErrorInvalidValue and,
where there is no GPU, every kernel path called with null device pointers hands the runtime's failure back."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_the_integer_launcher_reports_every_failure():
    subprocess.check_call(["make", "-C", CPP, "-f", "launch_status_int.mk", "launch_status_int"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(CPP, "launch_status_int")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "every call answered as expected" in p.stdout and "runtime error" not in p.stderr
    assert "dither, 24 -> 24" in p.stdout
