"""The 3D colour LUT's host side (ceracoder_amd/csrc/lut3d_host.c) under ASan + UBSan: a stand-alone program, csrc/san_lut3d_driver.c,
parses the golden .cube file, every truncation of it and over-long variants (a row too many, numbers of 400 digits, a line of 4000 blanks) from heap copies of
exactly their length into a buffer of exactly N^3 words, and runs the host rule at N = 2 and 65 on noise and at the ends of every clamp -- samples of 0 and 255
against tables of zeros, ones, noise and the identity, every matrix and range, strengths 1 and 256 -- into planes of exactly their size.  Host code only;
nothing is preloaded."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lut3d_small.cube")


def test_lut3d_host_side_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_lut3d"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_lut3d"), GOLDEN], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    size = os.path.getsize(GOLDEN)
    assert n["bad"] == 0 and n["parses"] == size + 10 and 1 < n["accepted"] < 40 and n["pictures"] == 2 * 4 * 4 * 2 * 2 * 5
