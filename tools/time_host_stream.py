"""PCIe-inclusive rate of the host boundary: mod_process_frame_host (synchronous) vs mod_submit/collect_frame_host
(MOD_PIPELINE_DEPTH frames in flight, pinned buffers), 1280x720, with and without the 32 B/px cloud coming back."""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moving_object_detector_amd import capi, synth
from moving_object_detector_amd.host_stream import HostStream
from moving_object_detector_amd.pipeline import Context

W, H, G, NF, CAP = 1280, 720, 4, 60, 64
cam, b = synth.make_batch(W, H, G, seed=0)
N = W * H
ctx = Context(W, H, max_frames=1)
ctx.set_camera(cam)
ctx.set_params(synth.Params())
tfs = capi.transforms_array(b["t"], b["q"])


ONLY = os.environ.get("ONLY")   # e.g. ONLY=pinned,nocloud,pipe for a profiler run
for use_pinned in ((True,) if ONLY else (False, True)):
    dn, dp, fl = ([ctx.pinned_copy(a).array for a in b[k][:G]] if use_pinned else b[k] for k in ("disparity_now", "disparity_prev", "flow"))
    n = C.c_int32(0)
    for want_cloud in ((False,) if ONLY else (True, False)):
        s = HostStream(ctx, capi.MOD_PIPELINE_DEPTH, CAP, outputs=("cloud", "labels") if want_cloud else ("labels",), fill=0, pinned=use_pinned)
        # synchronous
        t0 = time.perf_counter()
        for i in range(0 if ONLY else NF):
            f = i % G
            rc = ctx.lib.mod_process_frame_host(ctx.h, dn[f].ctypes.data, dp[f].ctypes.data, fl[f].ctypes.data, C.byref(tfs[f]), 0.1,
                                                s.cloud[0].ctypes.data if want_cloud else None, s.labels[0].ctypes.data, s.objects[0], CAP, C.byref(n))   # timed: the stream's own object array, no allocation per call
            assert rc == 0
        sync = NF / max(time.perf_counter() - t0, 1e-9)
        # pipelined
        t0 = time.perf_counter()
        for i in range(NF):
            f = i % G
            assert s.submit_frame(i % capi.MOD_PIPELINE_DEPTH, dn[f], dp[f], fl[f], tfs[f], 0.1) == 0
        s.finish()
        pipe = NF / (time.perf_counter() - t0)
        assert all(rc == 0 for rc in s.rc)
        mb = (16 + 4 + (32 if want_cloud else 0)) * N / 1e6
        print(f"host buffers {'pinned' if use_pinned else 'pageable'}, cloud back: {want_cloud}: {mb:.1f} MB per frame over PCIe; "
              f"synchronous {sync:.0f} frames/s, pipelined {pipe:.0f} frames/s ({pipe * mb / 1e3:.1f} GB/s), "
              f"objects in last frame {s.n[(NF - 1) % capi.MOD_PIPELINE_DEPTH]}")
ctx.close()
