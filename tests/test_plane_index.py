"""CPU: the one index rule of the encoder's residual planes (plane_index, alac_amd/csrc/alac_plane_index.hpp:
[sample / 4][stream][4]) compiled for the host in a stand-alone program of its own, built with the address and
undefined-behaviour sanitizers.  tests/cpp/plane_index.cpp enumerates samples j < 70 (72 with the rounding to whole cells) and
every stream of strides 64, 320 and 5 * 64: the map is a bijection onto [0, 4 * stride * ceil(rows / 4)), a group's four samples
are contiguous and 16-byte aligned, consecutive streams are 16 bytes apart."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_plane_index_is_a_bijection_of_aligned_groups():
    subprocess.check_call(["make", "-C", CPP, "-f", "plane_index.mk", "plane_index"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(CPP, "plane_index")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.splitlines()[-1] == "ok"
