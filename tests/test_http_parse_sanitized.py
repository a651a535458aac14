"""The HTTP wire parser under AddressSanitizer and UBSan, without Python.

``tests/native/http_parse_driver.cpp`` is a stand-alone program that includes
only ``gpushare_amd/native/http_parse.h``.  It parses a table of valid and
malformed responses whole, split in two at every offset and one byte at a
time, through heap copies of exactly each piece's size, and checks the
request-head builder byte for byte.  This test compiles it with
``-fsanitize=address,undefined -fno-sanitize-recover=all`` and runs the
binary: any out-of-bounds read, overflow or failed check is a non-zero exit.
"""

from __future__ import annotations

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "tests", "native", "http_parse_driver.cpp")
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# the runtimes linked into the binary where the static archives are
# installed: the program then does not care what else the loader brings in
STATIC = ["-static-libasan", "-static-libubsan"]


def _usable_sanitizer_flags(tmp_path):
    """The flag set with which an empty program links and runs, or None."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for extra in (STATIC, []):
        exe = tmp_path / "probe"
        r = subprocess.run(
            ["g++", *SAN_FLAGS, *extra, str(probe), "-o", str(exe)],
            capture_output=True, text=True,
        )
        if r.returncode != 0:
            continue
        if subprocess.run([str(exe)], capture_output=True).returncode == 0:
            return [*SAN_FLAGS, *extra]
    return None


def test_http_parse_driver_runs_clean_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = _usable_sanitizer_flags(tmp_path)
    if flags is None:
        pytest.skip("sanitizer runtime not linkable with this g++")
    exe = tmp_path / "http_parse_driver"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         *flags, DRIVER, "-o", str(exe)],
        capture_output=True, text=True,
    )
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run(
        [str(exe)], capture_output=True, text=True, timeout=120
    )
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.strip().endswith("OK"), run.stdout[-2000:]
