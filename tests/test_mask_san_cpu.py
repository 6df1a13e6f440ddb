"""The privacy masks' host side (ceracoder_amd/csrc/mask_host.c) under ASan + UBSan: a stand-alone program, csrc/san_mask_driver.c,
checks every field at both edges of its range and one step outside, runs the scalar rule -- on heap planes of exactly the visible size -- with every field at
its edges, with regions beyond every picture edge, on 16 x 16 and 8192 x 16 pictures and over 200 seeded random configurations, goes through every sum of
every radius of the blur's division, and runs the parser over its own strings, every truncation of one and junk.  The checksum it prints over every picture is
reproduced here by the numpy rule of tests/maskref.py from the same seed.  Host code only; nothing is preloaded."""
import json
import os
import subprocess

from tests import maskref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_mask_host_side_is_clean_under_asan_and_ubsan_and_equals_the_reference():
    r = subprocess.run(["make", "-C", CSRC, "san/san_mask"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_mask")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    want, pictures = R.driver_checksum()
    assert n["bad"] == 0 and n["checks"] == 6 * 4 - 1 + 5 + 10 + 5 and n["pictures"] == pictures == 6 * 2 + 5 * 2 + 2 + 13 * 2 + 2 * 3 + 200
    assert n["checksum"] == want, (n["checksum"], want)
