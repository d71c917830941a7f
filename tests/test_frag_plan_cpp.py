"""The frame map of IPv4 fragmentation (nsx_frag_count_host / nsx_frag_layout_host in
network-stack_amd/csrc/host_plan.cpp) built from source — with host_csum.cpp, which host_plan.cpp links against — under
AddressSanitizer + UBSan and driven by tests/cpp/test_frag_plan.cpp, a stand-alone program over the hand cases of
tests/test_frag_abi.py. CPU only: the unit includes no HIP header and needs neither the product library nor a GPU."""
import os
import subprocess

from conftest import ROOT

_SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_frag_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "test_frag_plan_san"
    csrc = os.path.join(ROOT, "network-stack_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "cpp", "test_frag_plan.cpp"),
                           os.path.join(csrc, "host_plan.cpp"), os.path.join(csrc, "host_csum.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=_SAN_ENV, timeout=120)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert out.stdout.strip().splitlines()[-1] == "OK"
