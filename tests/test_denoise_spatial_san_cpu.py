"""The rule of the spatial noise filter (ceracoder_amd/csrc/dspatial_host.c) under ASan + UBSan: a stand-alone program, csrc/san_dspatial_driver.c, asks
mi355enc_denoise_spatial_check for every range edge of every field (one step inside, one outside), builds the 33 tables, runs the filter and the measurement on
exactly-sized surfaces (every neighbour clamped, margins, a border, a visible part of one sample), and takes decisions at the ceilings of the measurement, from
both ends of the state, and 4000 seeded ones.  Host code only; nothing is preloaded."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_denoise_spatial_host_rule_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_dspatial"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_dspatial")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    assert n["bad"] == 0 and n["sets"] == 4000 and n["edges"] == 5 * 2 * 3 and n["tables"] == 33 and n["runs"] == 5 * 3 * 6 and n["decisions"] == 72 and n["refused"] == 12
