"""DevBuf, the owner of every device buffer (csrc/pmmg_devbuf.hpp), on the
host: tests/c/test_devbuf.cpp includes the header with a counting stub for the
two allocation calls and is built with ASan + UBSan, as the Medit fuzzer of
tests/test_medit.py is.  Nothing here needs a GPU or a HIP runtime."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_frees_what_it_owns(tmp_path):
    """ensure / release / move / swap / vectors that shrink: every block the
    stub handed out is freed exactly once and nothing is live at the end of a
    case (with an empty ~DevBuf the first case already fails: 32 bytes live)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = tmp_path / "test_devbuf"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", f"-I{os.path.join(REPO, 'parmmg_amd', 'csrc')}",
           "-o", str(exe), os.path.join(REPO, "tests", "c", "test_devbuf.cpp")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0 and "sanitize" in p.stdout:
        pytest.skip("sanitizer runtime not available: " + p.stdout[-200:])
    assert p.returncode == 0, p.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "all freed" in r.stdout
