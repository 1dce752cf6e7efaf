"""The host-side decisions of the interface displacement
(csrc/pmmg_moveifc_decide.hpp: the brake of a layer, the packing of the
colours) in a stand-alone program built with ASan + UBSan, as
tests/test_devbuf_host.py does for DevBuf.  Nothing here needs a GPU or a HIP
runtime."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_brake_and_packing_decisions(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = tmp_path / "test_moveifc_decide"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", f"-I{os.path.join(REPO, 'parmmg_amd', 'csrc')}",
           "-o", str(exe), os.path.join(REPO, "tests", "c", "test_moveifc_decide.cpp")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0 and "sanitize" in p.stdout:
        pytest.skip("sanitizer runtime not available: " + p.stdout[-200:])
    assert p.returncode == 0, p.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "all decided" in r.stdout
