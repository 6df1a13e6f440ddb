"""The parameter block of the HDR tone map (ceracoder_amd/csrc/hdr_host.c) under ASan + UBSan: a stand-alone program, csrc/san_hdr_driver.c, asks
mi355enc_hdr_tables for every edge of its argument range and builds the block for 3000 seeded parameter sets into a buffer of exactly its size.  Host code only."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_hdr_tables_are_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_hdr"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_hdr")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    assert n["bad"] == 0 and n["sets"] == 3000 and n["built"] > 100 and n["refused"] > 10000
