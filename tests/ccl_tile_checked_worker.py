"""Helper PROGRAM (not a test): runs the index-critical families of tests/ccl_tile_cases.py (full_requests, small_images, many_roots,
job_queue) through the clusterer of the library named by MOD_SF_LIB — the CHECKED build, whose kernels verify every data-derived index
before using it (csrc/mod_device.h MOD_CHECK; 12 = a link-request slot past the tile's share of the buffer, 13 = a root or halo
pixel outside the frame) — compares labels, cluster count and objects with the oracle, and prints the violation counters and the names
of the cases that differ as JSON.  Started by tests/test_gpu_ccl_tile_wide.py, once, before the product build sees these cases."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch

    import ccl_tile_cases as cc
    from moving_object_detector_amd import synth
    from moving_object_detector_amd.pipeline import PLANES, Context
    from oracle import pyoracle
    from test_gpu_cluster_stress import _make_cloud
    from util import compare_objects

    counters = np.zeros(96, np.uint64)
    ran, differ = [], []
    for case in cc.index_critical():
        W, H = case.W, case.H
        prm = synth.Params(cluster_size=case.cluster_size, neighbor_distance=case.n, depth_diff=cc.DEPTH_DIFF, dynamic_speed=0.3)
        planes = _make_cloud(W, H, case.dyn, case.z, np.random.default_rng(cc.seed_of(case)))
        ctx = Context(W, H, max_frames=1, max_objects=W * H // prm.cluster_size + 1)
        ctx.set_camera(synth.make_camera(W, H))
        ctx.set_params(prm)
        ws = ctx.workspace(1)
        for i, k in enumerate(PLANES):
            ws["planes"][i, 0].copy_(torch.from_numpy(planes[k]))
        for _ in range(2):                                   # twice: the second pass runs over scratch the first one left behind
            assert ctx.cluster(1, ws, mask_ready=False) == 0
            ctx.synchronize()
        counters[:] += ctx.debug_counters()
        rl, ro, rK = pyoracle.cluster(planes, prm, "tidy", max_objects=W * H // 2 + 16)
        try:
            assert int(ws["n_clusters"][0]) == rK
            assert np.array_equal(ws["labels"][0].cpu().numpy(), rl)
            compare_objects(ctx.objects_to_host(ws)[0], ro, strict_velocity=True)
        except AssertionError:
            differ.append(case.name)
        ctx.close()
        ran.append(case.name)
    print(json.dumps({"ran": ran, "differ": differ, "violations": {str(i - 64): int(v) for i, v in enumerate(counters) if i >= 64}}))


if __name__ == "__main__":
    main()
