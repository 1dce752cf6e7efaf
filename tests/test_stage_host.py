"""pmmg_stage.h, the device blocks of one call of the C host layer
(csrc/pmmg_host.c), on the host: tests/c/test_stage.c includes the header
against counting stubs of the six C-ABI calls it makes and is built with
ASan + UBSan, as tests/test_devbuf_host.py builds its program.  Nothing here
needs a GPU or a HIP runtime."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_frees_everything_and_latches_the_first_failure(tmp_path):
    """The sequence of pmmg_merge_grps (uploads without a source or without
    bytes, a room of 0 bytes, 3-wide and 6-wide rows through one reused block,
    downloads of 0 bytes), clean and with every allocation, copy and gather
    failing in turn: no device block stays live, no call follows the first
    failure, the host blocks handed out are the caller's (the leak check)."""
    cc = shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler found")
    exe = tmp_path / "test_stage"
    cmd = [cc, "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", f"-I{os.path.join(REPO, 'parmmg_amd', 'csrc')}",
           f"-I{os.path.join(REPO, 'include')}", "-o", str(exe), os.path.join(REPO, "tests", "c", "test_stage.c")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0 and "sanitize" in p.stdout:
        pytest.skip("sanitizer runtime not available: " + p.stdout[-200:])
    assert p.returncode == 0, p.stdout
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "23 runs, all freed" in r.stdout
