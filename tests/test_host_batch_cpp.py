"""The host batch driver (network-stack_amd/csrc/host_batch.cpp: shards over devices, the double-buffered chunk
pipeline, persistent staging buffers, error paths) with the rest of the C ABI's host code (csum_api.cpp, host_plan.cpp,
host_csum.cpp), built from source against a CPU model of the 13 HIP runtime calls it makes (tests/cpp/fake_hip.cpp) and
CPU stand-ins for the kernels (tests/cpp/cpu_launchers.cpp), and driven by tests/cpp/test_host_batch.cpp — once under
AddressSanitizer + UBSan, once under ThreadSanitizer, both with NSX_HOST_EXACT_BUFFERS so that every staging buffer is
exactly as large as reserve() asked. CPU only: a plain C++ compiler, the HIP headers for their types, no GPU and no
product library."""
import os
import subprocess

import pytest

from conftest import ROOT

_ROCM = os.environ.get("ROCM_PATH") or os.environ.get("ROCM") or "/opt/rocm"
_CSRC = os.path.join(ROOT, "network-stack_amd", "csrc")
_CPP = os.path.join(ROOT, "tests", "cpp")
_SOURCES = [os.path.join(_CPP, f) for f in ("test_host_batch.cpp", "fake_hip.cpp", "cpu_launchers.cpp")] + \
           [os.path.join(_CSRC, f) for f in ("host_batch.cpp", "csum_api.cpp", "host_plan.cpp", "host_csum.cpp")]
_FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DNSX_HOST_EXACT_BUFFERS",
          "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(_ROCM, "include"), "-fno-omit-frame-pointer", "-pthread"]
# NSX_HOST_COPY_THREADS=3: the program's 4 MiB + 4097 B spans split unevenly in both directions of stage_copy
_ENV = dict(os.environ, NSX_HOST_COPY_THREADS="3", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
            UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1")


def _build_and_run(tmp_path, sanitize):
    exe = tmp_path / "test_host_batch_san"
    subprocess.check_call(["g++"] + _FLAGS + sanitize + _SOURCES + ["-o", str(exe)])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, env=_ENV,
                         timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-6000:])
    assert out.stdout.strip().splitlines()[-1] == "OK"


def test_host_batch_under_asan_ubsan(tmp_path):
    _build_and_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_host_batch_under_tsan(tmp_path):
    probe = tmp_path / "tsan_probe"
    (tmp_path / "tsan_probe.cpp").write_text("int main() { return 0; }\n")
    subprocess.check_call(["g++", "-fsanitize=thread", str(tmp_path / "tsan_probe.cpp"), "-o", str(probe)])
    started = subprocess.run([str(probe)], capture_output=True, text=True, timeout=60)
    if started.returncode != 0:  # e.g. an address-space layout the sanitizer's runtime cannot map
        pytest.skip("an empty program built with -fsanitize=thread does not start on this host: " +
                    (started.stderr.strip().splitlines() or ["exit %d" % started.returncode])[-1])
    _build_and_run(tmp_path, ["-fsanitize=thread"])
