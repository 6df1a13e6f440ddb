"""Region-of-interest quantisation's host side (ceracoder_amd/csrc/roi_host.c) under ASan + UBSan: a stand-alone program,
csrc/san_roi_driver.c, checks every field at both edges of its range and one step outside, makes the map -- into heap buffers of exactly mbw mbh bytes -- with
every field at its edges, with rectangles beyond every picture edge, at 1 x 1 and 512 x 512 macroblocks and over 200 seeded random configurations, and runs the
parser over its own strings, every truncation of one and junk.  The checksum it prints over every map is reproduced here by the numpy rule of tests/roiref.py
from the same seed.  Host code only; nothing is preloaded."""
import json
import os
import subprocess

from tests import roiref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_roi_host_side_is_clean_under_asan_and_ubsan_and_equals_the_reference():
    r = subprocess.run(["make", "-C", CSRC, "san/san_roi"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_roi")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    want, maps = R.driver_checksum()
    assert n["bad"] == 0 and n["checks"] == 8 * 4 + 1 and n["maps"] == maps == 8 * 2 * 2 + 12 * 3 + 6 + 200
    assert n["checksum"] == want, (n["checksum"], want)
