"""The PAM reader of the image layers (ceracoder_amd/csrc/image_host.c) under ASan + UBSan: a stand-alone program, csrc/san_image_driver.c, feeds it every
prefix of two valid files and each file with every header byte replaced by each of 0, '9', ' ', a line feed and 0xFF.  Host code only."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ceracoder_amd", "csrc")


def test_pam_reader_is_clean_under_asan_and_ubsan():
    r = subprocess.run(["make", "-C", CSRC, "san/san_image"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "san", "san_image")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    n = json.loads(r.stdout)
    # every prefix but the whole file is refused; of the damaged headers only those whose damage lies in a comment or leaves a valid header pass
    assert n["ok"] >= 2 and n["err"] > n["ok"]
