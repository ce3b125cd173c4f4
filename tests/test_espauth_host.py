"""host/esp_sa.hh (SHA-1 compression, HMAC midstates, the SA image and its
refusals) under AddressSanitizer + UndefinedBehaviorSanitizer: the stand-alone
program tests/esp_sa_check.cc, CPU only, no library loaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_esp_sa_under_asan_ubsan(tmp_path):
    exe = tmp_path / "esp_sa_check"
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", os.path.join(ROOT, "tests", "esp_sa_check.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "esp_sa_check ok" in out.stdout, out.stdout + out.stderr[-4000:]
