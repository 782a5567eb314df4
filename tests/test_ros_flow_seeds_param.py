"""CPU: the constructor node reads `~flow_seeds` (default 1: off) before its first submit and hands it to the host mirror, which hands it
to the C ABI.  A syntax pin in the manner of tests/test_ros_disparity_filter_params.py: the node still compiles against the
declaration-only ROS stand-ins."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "moving_object_detector_amd", "host")
NODE = os.path.join(HOST, "ros_adapter", "scene_flow_constructor", "src", "scene_flow_constructor_node.cpp")


def test_node_reads_the_parameter_with_default_one_before_any_submit():
    src = open(NODE).read()
    m = re.search(r'impl_->setFlowPropagation\(private_node_handle_\.param\("(\w+)",\s*(\w+)\)\);', src)
    assert m, "the node does not call setFlowPropagation"
    assert m.groups() == ("flow_seeds", "1")
    first_submit = min(src.index(s) for s in ("impl_->submitStereo(", "impl_->submitOdometry(") if s in src)
    assert m.start() < first_submit                              # in the constructor, ahead of the callback that submits
    assert "~flow_seeds" in src                                  # and in the header comment's list of parameters


def test_host_mirror_passes_it_to_the_c_abi():
    src = open(os.path.join(HOST, "scene_flow_constructor.hpp")).read()
    m = re.search(r"void setFlowPropagation\(int seeds\)\s*\{(.*?)\}", src, flags=re.S)
    assert m, "SceneFlowConstructor::setFlowPropagation(int) is missing"
    assert "mod_set_flow_propagation(ctx_, seeds)" in m.group(1)


def test_node_compiles_against_the_ros_stand_ins():
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "ros_stubs"),
                        "-I", os.path.join(ROOT, "include"), "-I", HOST, NODE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]


def test_integration_guide_names_it():
    assert "~flow_seeds" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
