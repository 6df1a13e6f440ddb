"""The writer of the JPEG stills (ceracoder_amd/csrc/snapshot_host.c) under ASan + UBSan: a stand-alone program, csrc/san_snapshot_driver.c, runs it over random
and extreme level sets, with and without the per-block hints, into every capacity from nothing to the file's length, and back through the product's decoder.
Host code only; nothing is loaded into Python under a sanitizer."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_still_writer_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_snapshot"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_snapshot")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    assert n["files"] == 3 * 4 * 2 * 3 and n["refused"] == 3 * 2 * 3 and n["caps"] > 10000
