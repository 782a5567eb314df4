"""CPU: what the C++ host mirror (host/scene_flow_constructor.hpp, host/clusterer_nodelet.hpp) asks of the C ABI, call by call.
tests/cpp/mirror_calls_test.cpp links no library: it defines ModContext as a call recorder and a stub for every mod_* function the two
headers call, runs the four submits, construct / stereoCallback, the collects, the reconfigure callbacks and the clusterer through
their scenarios on a 4 x 3 camera and logs every call with its arguments (which buffer each pointer is), the value returned and what
the caller can see afterwards.  The log is compared byte for byte with tests/golden/mirror_calls.txt, which was recorded with the
headers as they were before the submits were folded into one frame path: the order of the calls, their arguments, the slot ring, the
stamp / dt rule and the messages of the mirror are pinned without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirror_calls_match_the_recorded_log(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "mirror_calls_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "mirror_calls_test.cpp"), "-o", exe])
    got = subprocess.run([exe], stdout=subprocess.PIPE, check=True, timeout=60).stdout
    with open(os.path.join(ROOT, "tests", "golden", "mirror_calls.txt"), "rb") as f:
        want = f.read()
    assert b"?" not in got, "a pointer that no scenario registered reached the library"
    if got != want:
        g, w = got.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        context = "\n".join(g[max(0, first - 6):first])
        pytest.fail("the log differs from tests/golden/mirror_calls.txt at line %d (%d lines against %d)\nbefore:\n%s\ngot:  %s\nwant: %s"
                    % (first + 1, len(g), len(w), context, g[first] if first < len(g) else "<end>", w[first] if first < len(w) else "<end>"))
