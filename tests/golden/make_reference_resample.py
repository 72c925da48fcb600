#!/usr/bin/env python3
"""Golden vectors of the reference's own resampler (reference MBExWN_NVoc/sig_proc/resample.py:7-64, the function its
bin/generate_mel.py:58-59 calls): ``resample(x, in_sr, 24000, axis=0)`` on seeded float32 noise.

The module is imported by path, at generation time only, in this process; before the import ``np.int`` and ``np.math`` are
set, because the reference uses both names and current numpy has neither.

Keys: "sr<in_sr>_n<n>/x" (float32 input), ".../y" (float32 output) and "sr<in_sr>/taps" (the reference's float32 filter,
once per rate; none for 12345 Hz, whose 72 000 taps are 288 KB -- the design is pinned by the other rates).
Writes tests/golden/reference_resample.npz.

usage: make_reference_resample.py <directory of the reference tree>
"""
import importlib.util
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_SR = 24000
CASES = ((48000, 1), (48000, 2), (48000, 777), (44100, 1000), (16000, 301), (22050, 500), (8000, 100), (32000, 1023),
         (96000, 900), (11025, 200), (12345, 400))
NO_TAPS = (12345,)


def case_input(in_sr, n):
    return np.random.default_rng(in_sr * 10007 + n).standard_normal(n).astype(np.float32)


def main(reference_root):
    np.int = int
    np.math = math
    spec = importlib.util.spec_from_file_location(
        "reference_resample", os.path.join(reference_root, "MBExWN_NVoc", "sig_proc", "resample.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    out = {}
    for in_sr, n in CASES:
        x = case_input(in_sr, n)
        y, taps = module.resample(x, in_sr, OUT_SR, axis=0)
        assert y.dtype == np.float32 and taps.dtype == np.float32
        out[f"sr{in_sr}_n{n}/x"] = x
        out[f"sr{in_sr}_n{n}/y"] = y
        if in_sr not in NO_TAPS:
            out[f"sr{in_sr}/taps"] = taps
        print(in_sr, n, y.shape, taps.shape)
    np.savez_compressed(os.path.join(HERE, "reference_resample.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
