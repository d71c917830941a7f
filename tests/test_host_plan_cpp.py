"""The host batch calls' planning unit (network-stack_amd/csrc/host_plan.cpp: chunk cuts, shard bounds, the sender
job's staging layout, the frame-map and layout validators) built from source — with host_csum.cpp for shard_plan —
under AddressSanitizer + UBSan and driven by tests/cpp/test_host_plan.cpp. CPU only: the unit includes no HIP header
and needs neither the product library nor a GPU."""
import os
import subprocess

from conftest import ROOT

_SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_host_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "test_host_plan_san"
    csrc = os.path.join(ROOT, "network-stack_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "cpp", "test_host_plan.cpp"),
                           os.path.join(csrc, "host_plan.cpp"), os.path.join(csrc, "host_csum.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=_SAN_ENV, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.strip().splitlines()[-1] == "OK"
