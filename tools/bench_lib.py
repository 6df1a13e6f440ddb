#!/usr/bin/env python3
"""bench.py against another build of the library (A/B runs of kernel variants inside ONE gpurun call -- boxes differ by
several per cent, so numbers from different calls do not compare):  MI355ENC_LIB=/path/libmi355enc_x.so python tools/bench_lib.py [bench.py flags]
MI355ENC_BENCH_ROI="x,y,w,h,delta[,feather];..." (and MI355ENC_BENCH_ROI_BALANCE=n): every encoder the benchmark opens gets that region of interest
(mi355enc_set_roi) before its first picture -- the benchmark itself knows no such option."""
import os, sys, subprocess
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ceracoder_amd import enc as E
E.LIB_PATH = os.environ.get("MI355ENC_LIB", E.LIB_PATH)
if os.environ.get("MI355ENC_BENCH_ROI"):
    _open = E.Encoder.__init__

    def _open_with_roi(self, *a, **kw):
        _open(self, *a, **kw)
        self.set_roi(E.roi_parse(os.environ["MI355ENC_BENCH_ROI"], int(os.environ.get("MI355ENC_BENCH_ROI_BALANCE", "0"))))
    E.Encoder.__init__ = _open_with_roi
import runpy
sys.argv = ["bench.py"] + sys.argv[1:]
runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"), run_name="__main__")
