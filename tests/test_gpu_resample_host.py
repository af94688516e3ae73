"""GPU: alac_hip_resample_int_host / alac_hip_resample_float_host called from C++ (tests/cpp/resample.cpp): a 16-bit interleaved
stereo plane and a float32 planar one, two segments each, give the rows and the reports the Python side recorded from the
device forms, bit for bit, and those lie within the accepted distance of the restatement (tests/resample_ref.py)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import alac_amd
import resample_ref as rr

pytestmark = pytest.mark.gpu

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


@pytest.fixture(scope="module")
def harness(gpu_ctx):
    subprocess.check_call(["make", "-C", CPP, "-f", "resample.mk", "resample"], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "resample")


@pytest.mark.parametrize("kind,rates", [("int", (44100, 48000)), ("float", (96000, 44100))])
def test_host_forms_from_cpp(gpu_ctx, harness, tmp_path, kind, rates):
    frames, cut = 2345, 1001
    L, M, coefs = alac_amd.resample_filter(*rates)
    rng = np.random.default_rng(7)
    if kind == "int":
        s = rng.integers(-30000, 30000, (frames, 2)).astype(np.int16)  # interleaved
        (tmp_path / "in").write_bytes(s.tobytes())
        x = s.T.astype(np.float64) * 2.0 ** -15
        y, rep = gpu_ctx.resample_int(torch.from_numpy(s).to(gpu_ctx.device).t(), rates[0], rates[1], seg_first_frame=[0, cut, frames])
    else:
        f = rng.uniform(-1.2, 1.2, (2, frames)).astype(np.float32)  # planar
        f[1, 17] = np.nan
        (tmp_path / "in").write_bytes(f.tobytes())
        x = np.where(np.isfinite(f), f.astype(np.float64), 0.0)
        y, rep = gpu_ctx.resample_float(torch.from_numpy(f).to(gpu_ctx.device), rates[0], rates[1], seg_first_frame=[0, cut, frames])
    gpu_ctx.synchronize()
    want, reports = y.cpu().numpy(), alac_amd.Context.resample_reports(rep)
    p = subprocess.run([harness, kind, str(rates[0]), str(rates[1]), str(frames), str(cut), str(tmp_path / "in"), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = p.stdout.split("\n")
    total = rr.out_frames(cut, L, M) + rr.out_frames(frames - cut, L, M)
    assert lines[2] == "total %d" % total
    got = np.frombuffer((tmp_path / "out").read_bytes(), np.float32).reshape(2, total)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for s, r in enumerate(reports):
        first, n, peak, bad = lines[s].split()
        assert (int(first), int(n), float(peak), int(bad)) == (r.out_first, r.out_frames, r.peak, r.nonfinite)
    assert [r.nonfinite for r in reports] == ([0, 0] if kind == "int" else [1, 0])
    ref = rr.resample(x.T, L, M, coefs, [0, cut, frames]).T
    assert (np.abs(got - ref) <= rr.accepted(ref, rr.bound(coefs, np.abs(x).max()))).all()
