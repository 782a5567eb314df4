"""Writes tests/golden/flow/flow_prop_320x240.npz: two image pairs (moving textured boxes,
moving_object_detector_amd.synth.make_moving_images) and the flow of the numpy restatement WITH neighbour-seed propagation
(tests/models/flow_prop_model.py, seeds = 5) — one with the sub-pixel step and the forward-backward check on, one with both off.  The
fixture pins the model against drift; tests/test_flow_prop_model.py and tests/test_gpu_flow_prop.py read it.  Run from the repository
root:
    python tests/golden/make_flow_prop_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "models"))

import flow_prop_model as fp  # noqa: E402
from moving_object_detector_amd import synth  # noqa: E402

W, H = 320, 240
SEEDS = 5
PARAMS = [(4, 4, 5, 1, 1), (4, 4, 5, 0, -1)]      # levels, radius, window, subpixel, fb_check


def main():
    prev, now, flow = [], [], []
    for k, prm in enumerate(PARAMS):
        m = synth.make_moving_images(W, H, seed=40 + k, n_boxes=3, shift=(4, 12))
        prev.append(m["left0"]); now.append(m["left1"])
        flow.append(fp.flow(m["left0"], m["left1"], fp.FlowParams(*prm), SEEDS))
    np.savez_compressed(os.path.join(HERE, "flow", "flow_prop_320x240.npz"), pairs=np.int32(len(PARAMS)), seeds=np.int32(SEEDS),
                        params=np.array(PARAMS, np.int32), prev=np.stack(prev), now=np.stack(now), flow=np.stack(flow))


if __name__ == "__main__":
    main()
