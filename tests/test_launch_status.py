"""The launcher convention of alac_amd/csrc: every function that enqueues work returns hipError_t, the
status of the first runtime call or kernel launch in it that failed.  Checked on the sources (no status is discarded, no
launcher is void, kernels are launched from one helper only) and, where there is no GPU, by calling every launcher once
(tests/cpp/launch_status.hip): each must hand the failure back."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alac_amd", "csrc")
CPP = os.path.join(ROOT, "tests", "cpp")

# teardown paths: nobody is left to tell, and the next step must run whatever this one said
TEARDOWN = re.compile(r"hip(\w*Destroy|Free|HostFree|SetDevice|StreamSynchronize)$")
DISCARDS_ALLOWED = {
    ("alac_capi.hip", "alac_hip_destroy"): TEARDOWN,
    ("alac_capi.hip", "upload_segment_table"): re.compile(r"hipHostFree$"),
    ("alac_host.hpp", "~DevBuf"): re.compile(r"hipFree$"),
    ("alac_comm.cpp", "alac_hip_comm_destroy"): TEARDOWN,
    # hipPointerGetAttributes on plain host memory leaves an error behind that is none
    ("alac_matrix.hip", "on_device"): re.compile(r"hipGetLastError$"),
}
HELPER = ("alac_kernels.hpp", "launch_kernel_lds")  # launch_kernel is this one with no dynamic LDS
LAST_ERROR_ALLOWED = {HELPER, ("alac_matrix.hip", "on_device")}


def sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".hpp", ".cpp", ".h", ".c")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read().split("\n")


def code_of(line):
    return line.split("//", 1)[0]


def enclosing_function(lines, i):
    """Name of the function whose body holds line i.  A body opens with a brace on a line of its own, at the indentation of
    the declaration in front of it: column 0, or 4 for a member function defined in its class."""
    member = True
    for j in range(i - 1, 0, -1):
        if lines[j] == "}":
            return None  # behind the end of a function
        if lines[j].startswith("    }"):
            member = False  # a block closed at this depth: line i is in a free function
        if lines[j] == "{" or (member and lines[j] == "    {"):
            indent = len(lines[j]) - 1
            k = j - 1
            while k > 0 and lines[k][indent:indent + 1] in (" ", ""):  # continuation lines of the declaration
                k -= 1
            m = re.search(r"(~?\w+)\s*\(", lines[k])
            return m.group(1) if m else None
    return None


def occurrences(pattern):
    rx = re.compile(pattern)
    for name, lines in sources():
        for i, line in enumerate(lines):
            for m in rx.finditer(code_of(line)):
                yield name, enclosing_function(lines, i), m, "%s:%d: %s" % (name, i + 1, line.strip())


def test_no_status_is_discarded():
    bad = []
    for name, func, m, where in occurrences(r"\(void\)\s*(hip\w+)\s*\("):
        allowed = DISCARDS_ALLOWED.get((name, func))
        if not (allowed and allowed.match(m.group(1))):
            bad.append(where)
    assert not bad, "\n".join(bad)


def test_every_launcher_returns_a_status():
    seen, bad = 0, []
    for name, lines in sources():
        if name not in ("alac_kernels.hpp", "alac_encode_v1_types.hpp", "alac_encode_v1_impl.hpp"):
            continue
        for i, line in enumerate(lines):
            m = re.match(r"(?:static |inline )*([\w:]+) (launch_\w+|v1c_\w+)\(", line)
            if m:
                seen += 1
                if m.group(1) != "hipError_t":
                    bad.append("%s:%d: %s" % (name, i + 1, line.strip()))
    assert seen >= 30, seen  # the declarations are found at all
    assert not bad, "\n".join(bad)


def test_kernels_are_launched_from_the_helper_only():
    launches = [(name, func, where) for name, func, _, where in occurrences(r"hipLaunchKernelGGL|<<<")]
    assert [(n, f) for n, f, _ in launches] == [HELPER], "\n".join(w for _, _, w in launches)
    reads = [(name, func, where) for name, func, _, where in occurrences(r"hipGetLastError")]
    assert reads and all((n, f) in LAST_ERROR_ALLOWED for n, f, _ in reads), "\n".join(w for _, _, w in reads)


def test_every_launcher_reports_a_failed_call():
    subprocess.check_call(["make", "-C", CPP, "launch_status"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(CPP, "launch_status")], capture_output=True, text=True, timeout=120)
    if p.returncode == 77:
        pytest.skip("a GPU is present: the program calls the launchers with null device pointers")
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "every call reported a failure" in p.stdout
