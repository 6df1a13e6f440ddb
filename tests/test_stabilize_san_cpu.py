"""The stabiliser's rule (ceracoder_amd/csrc/stab_host.c) under ASan + UBSan: a stand-alone program, csrc/san_stab_driver.c, asks
mi355enc_stabilize_check for every range edge of every field, projects 200 seeded planes (both byte steps, odd sizes, stride slack) into buffers of exactly
their size, votes at n = 4 range for every range and at the ceiling of the sums (the 33-bit cost), and steps the trajectory over negative and positive states
for every leak edge against long arithmetic with an explicit floor.  Host code only; nothing is preloaded."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_stabilize_rule_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_stab"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_stab")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    assert n["bad"] == 0 and n["edges"] == 4 * 2 * 5 and n["planes"] == 200 and n["votes"] == 33 and n["steps"] == 6 * 5 * 2000
