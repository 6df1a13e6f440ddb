"""The rule of the frame-rate conversion (ceracoder_amd/csrc/rate_host.c) under ASan + UBSan: a stand-alone program, csrc/san_rate_driver.c, runs the plan over
seeded pts sequences -- anchors near +-2^62, pts_per_second 1 .. 10^9, rates 1/1 .. 240000/1001, jitter, holes, backward steps.  Host code only."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_rate_plan_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_rate"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_rate")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    assert n["bad"] == 0 and n["sequences"] == 3000
    assert min(n["dropped"], n["multi"], n["blended"], n["resyncs"]) > 1000 and n["out"] > 100000
