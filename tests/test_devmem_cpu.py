"""csrc/rt_devmem.h, the owner of the context's device buffers, on the CPU: tests/devmem_main.cpp
instantiates it over a malloc backend with live counters and a switch that fails the k-th allocation,
built with ASan + UBSan as a stand-alone program (a double free, a leak through the registry or a
dereferenced null epoch ends it with a non-zero status)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_memory_owner_under_sanitizers(tmp_path):
    exe = tmp_path / "devmem_main"
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "esctp1raytracer_amd", "csrc"),
                        os.path.join(ROOT, "tests", "devmem_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "failures=0" in r.stdout
