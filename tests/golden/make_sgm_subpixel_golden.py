#!/usr/bin/env python3
"""Generates tests/golden/sgm_subpixel_160x96.npz: one slanted stereo pair (synth.make_slanted_stereo) and what the model of the SGM
estimator's sub-pixel mode (tests/models/sgm_subpixel_model.py) makes of it, with and without the fraction.  Build-defined vectors,
like sgm_320x240.npz.  Run from the repo root:  python tests/golden/make_sgm_subpixel_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "models"))
import sgm_subpixel_model as sm  # noqa: E402
from moving_object_detector_amd import synth  # noqa: E402

W, H, D, SEED, D_TOP, D_BOTTOM = 160, 96, 48, 21, 4.0, 37.0
left, right, truth = synth.make_slanted_stereo(W, H, SEED, D_TOP, D_BOTTOM)
sub = sm.compute_images(left, right, D)
whole = sm.compute_images(left, right, D, fraction_bits=0)
np.savez_compressed(os.path.join(HERE, "sgm_subpixel_160x96.npz"), left=left, right=right, seed=np.int32(SEED), d_top=np.float32(D_TOP),
                    d_bottom=np.float32(D_BOTTOM), D=np.int32(D), P1=np.int32(6), P2=np.int32(96), paths=np.int32(8), lr_check=np.int32(1),
                    median=np.int32(1), fraction_bits=np.int32(sm.FRACTION_BITS), disparity=sub, disparity_integer=whole)
v = (sub >= 0) & (whole >= 0)
print(f"sgm_subpixel_160x96: valid {v.mean():.3f}, MAE {np.abs(whole - truth)[v].mean():.4f} px integer, {np.abs(sub - truth)[v].mean():.4f} px sub-pixel")
