#!/usr/bin/env python3
"""bench.py with the same arguments, followed on stderr by what the classifier preparation decided in that process:
prepare.site_report() and, per accepted 1x1 backward-data site, its shape and its walk (bench.py itself prints neither).
usage: python profiles/bench_site_report.py --gpus 1 --steps 3 --warmup 1"""
import atexit
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "image-classification-xai_amd"))


def report():
    from xai_engine import prepare
    print("site report: " + prepare.site_report(), file=sys.stderr)
    for weight, shape, walk in prepare.CONV_SITE_COUNTS["walks"]:
        print(f"  1x1 backward-data {weight} on input {shape}: walk {walk}", file=sys.stderr)
    for weight, shape, walk in prepare.CONV_WIDE_SITE_COUNTS["walks"]:
        print(f"  1x1 backward-data on large planes {weight} on input {shape}: walk {walk}", file=sys.stderr)


atexit.register(report)
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(sys.argv[0], run_name="__main__")
