"""CPU: the wire formats of sensor_msgs/Image and visualization_msgs/MarkerArray (host/ros_wire.hpp) against hand-written buffers:
tests/cpp/ros_wire_markers_test.cpp, compiled the way tests/test_host_wire.py compiles its program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_and_marker_array_wire_format(tmp_path):
    exe = str(tmp_path / "ros_wire_markers_test")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "ros_wire_markers_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "ok: Image 48 bytes, MarkerArray 209 bytes"
