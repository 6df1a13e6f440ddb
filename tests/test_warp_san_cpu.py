"""The mesh warp's rule (ceracoder_amd/csrc/warp_host.c) under ASan + UBSan: a stand-alone program, csrc/san_warp_driver.c, asks for the
whole coefficient table, runs the builder at every range edge of every parameter (alone, and with every other parameter at its lower or upper edge) at 2 x 2,
64 x 48 and 8192 x 16 into meshes of exactly their size, and warps seeded noise at the four picture sizes through the six named sets, a folded mesh and meshes
at the ends of the node range (the interpolation at its ceiling below 2^31), both filters, into planes of exactly their size.  Host code only; nothing is
preloaded."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_warp_rule_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_warp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_warp")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)  # (built: the sets the builder accepted -- at 64 x 48 alone every in-range edge value of a single parameter, 7 x 2 x 3, builds)
    assert n["bad"] == 0 and n["coeffs"] == 64 and n["edges"] == 3 * 7 * 2 * 5 * 3 and n["built"] >= 42 and n["pictures"] == 4 * 10 * 2
