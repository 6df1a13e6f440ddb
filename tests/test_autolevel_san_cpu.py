"""The rule of automatic levels and white balance (ceracoder_amd/csrc/autolevel_host.c) under ASan + UBSan: a stand-alone program,
csrc/san_autolevel_driver.c, asks mi355enc_autolevel_check for every range edge of every field (one step inside, one outside), takes decisions there at the
ceilings of the measurement and from every end of the state, and 4000 seeded ones, into a state, a record and a table of exactly their size.  Host code only;
nothing is preloaded."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_autolevel_decide_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_autolevel"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_autolevel")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    assert n["bad"] == 0 and n["sets"] == 4000 and n["edges"] == 7 * 2 * 3 and n["decisions"] == 28 * 32 and n["refused"] == 14 * 32 + 18
