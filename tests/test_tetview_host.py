"""tet_view, the one decode-and-check of an entry point's (ne, tetv, adja, tet8)
(csrc/pmmg_tetview.hpp), on the host: tests/c/test_tetview.cpp walks packed and
separate arrays, each array NULL under each caller's policy, ne around 2^29 and
every base off its 16-byte line, on fabricated pointers, built with ASan +
UBSan as tests/test_devbuf_host.py builds its program.  Nothing here needs a
GPU or a HIP runtime."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tetview_codes_and_views(tmp_path):
    """every case's returned code and filled view (a check that forgot the
    bound, the alignment of one base or a caller's policy fails a named case)"""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = tmp_path / "test_tetview"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", f"-I{os.path.join(REPO, 'parmmg_amd', 'csrc')}",
           "-o", str(exe), os.path.join(REPO, "tests", "c", "test_tetview.cpp")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0 and "sanitize" in p.stdout:
        pytest.skip("sanitizer runtime not available: " + p.stdout[-200:])
    assert p.returncode == 0, p.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "all views as expected" in r.stdout
