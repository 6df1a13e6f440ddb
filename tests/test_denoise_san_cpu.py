"""The rule of the temporal noise filter (ceracoder_amd/csrc/denoise_host.c) under ASan + UBSan: a stand-alone program, csrc/san_denoise_driver.c, asks
mi355enc_denoise_check and mi355enc_denoise_tables for both strengths at each range edge (one step inside, one outside) and builds the tables for 4000 seeded
parameter sets into buffers of exactly 256 bytes.  Host code only; nothing is preloaded."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_denoise_tables_are_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_denoise"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_denoise")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    assert n["bad"] == 0 and n["sets"] == 4000 and n["edges"] == 2 * 2 * 3 * 3 and n["refused"] == 12
