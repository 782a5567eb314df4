#!/usr/bin/env python3
"""Generates tests/golden/sgm_filters_160x96.npz: the committed slanted stereo pair (sgm_subpixel_160x96.npz) and what the model of the
SGM estimator's rejection filters (tests/models/sgm_filters_model.py) makes of it with both filters on, as integer and as sub-pixel
disparity.  Build-defined vectors, like sgm_subpixel_160x96.npz.  Run from the repo root:  python tests/golden/make_sgm_filters_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "models"))
import sgm_filters_model as fm  # noqa: E402

UNIQUENESS, SPECKLE_SIZE, SPECKLE_RANGE = 10, 100, 1
g = np.load(os.path.join(HERE, "sgm_subpixel_160x96.npz"))
left, right, D = g["left"], g["right"], int(g["D"])
f = dict(uniqueness_ratio=UNIQUENESS, speckle_size=SPECKLE_SIZE, speckle_range=SPECKLE_RANGE)
whole = fm.compute_images(left, right, D, fraction_bits=0, **f)
sub = fm.compute_images(left, right, D, fraction_bits=4, **f)
np.savez_compressed(os.path.join(HERE, "sgm_filters_160x96.npz"), left=left, right=right, D=np.int32(D), P1=np.int32(6), P2=np.int32(96),
                    paths=np.int32(8), lr_check=np.int32(1), median=np.int32(1), uniqueness_ratio=np.int32(UNIQUENESS),
                    speckle_size=np.int32(SPECKLE_SIZE), speckle_range=np.int32(SPECKLE_RANGE), disparity=sub, disparity_integer=whole)
for name, got, ref in (("integer", whole, g["disparity_integer"]), ("sub-pixel", sub, g["disparity"])):
    print(f"sgm_filters_160x96 {name}: valid {(ref >= 0).mean():.3f} unfiltered, {(got >= 0).mean():.3f} filtered")
