"""The inflate core of k_inflate (csrc/inflate_core.h) on the CPU under ASan + UBSan:
tools/sanitize/inflate_host runs it over every vector of tools/rawdeflate.py and 20 000 fixed-seed
single-byte mutations, and compares output and verdict with zlib's gzip mode; the loop iterations
must stay within 8 * src_len + dlen + a constant (termination by construction). A stand-alone
program: no kernel launch, nothing loaded into Python."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tools", "sanitize")


def test_inflate_core_against_zlib(tmp_path):
    r = subprocess.run(["make", "-s", "-C", SAN, "build/inflate_host"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rawdeflate.py"), "--dump", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(SAN, "build", "inflate_host"), str(tmp_path)], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                                             UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
