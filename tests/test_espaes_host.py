"""host/aes_key.hh (GF(2^8) tables, the AES-128 key expansion, the decryption
round keys, the SA image and its refusals) under AddressSanitizer +
UndefinedBehaviorSanitizer: the stand-alone program tests/aes_key_check.cc,
CPU only, no library loaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_aes_key_under_asan_ubsan(tmp_path):
    exe = tmp_path / "aes_key_check"
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", os.path.join(ROOT, "tests", "aes_key_check.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "aes_key_check ok" in out.stdout, out.stdout + out.stderr[-4000:]
