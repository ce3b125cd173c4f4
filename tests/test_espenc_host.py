"""The encryption half of host/aes_key.hh (Te0, the encryption round keys,
encrypt_block, the two-image build) under AddressSanitizer +
UndefinedBehaviorSanitizer: the stand-alone program tests/aes_enc_key_check.cc,
CPU only, no library loaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_aes_enc_key_under_asan_ubsan(tmp_path):
    exe = tmp_path / "aes_enc_key_check"
    subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                    "-O1", "-std=c++17", os.path.join(ROOT, "tests", "aes_enc_key_check.cc"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "aes_enc_key_check ok" in out.stdout, out.stdout + out.stderr[-4000:]
