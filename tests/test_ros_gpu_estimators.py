"""CPU: the constructor node runs every estimator on the GPU by default — `~gpu_estimators` (default true) submits through the host
mirror's submitOdometry with the layout taken from the message, publishes ~optical_flow for subscribers, and broadcasts
odom -> base_link with the reference's frame parameters and base -> camera TF lookup; `~crop_width` / `~crop_height` replace the
image_crop nodes; tf2_ros is in both manifests.  Source-level pins; the shell itself compiles in test_ros_adapter_syntax.py."""
import os
import re
import xml.dom.minidom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "moving_object_detector_amd", "host", "ros_adapter", "scene_flow_constructor")
NODE = os.path.join(PKG, "src", "scene_flow_constructor_node.cpp")
MIRROR = os.path.join(ROOT, "moving_object_detector_amd", "host", "scene_flow_constructor.hpp")


def test_gpu_estimators_parameter_and_path():
    src = open(NODE).read()
    assert 'param("gpu_estimators", true)' in src
    assert "if (gpu_estimators_) { gpuCallback(" in src
    assert "impl_->submitOdometry(" in src and "impl_->collectOdometry(" in src
    assert "o.encoding = m.encoding; o.step = (int)m.step;" in src            # encoding and step from the message
    assert "mod_host::image_encoding(left_image->encoding) >= 0" in src and "frame dropped" in src
    assert re.search(r"want_flow = optflow_pub_\.getNumSubscribers\(\) > 0", src)
    # the CALL-OUT path stays for ~gpu_estimators:=false
    assert "estimateOpticalFlow" in src and "estimateCameraMotion" in src and "CALL-OUT" in src


def test_layout_call_in_the_mirror():
    src = open(MIRROR).read()
    assert "mod_set_image_layout(ctx_, &lay)" in src
    body = src[src.index("int submitOdometry("):]
    assert "useLayout(*left_image, *right_image, x0, y0)" in body[:2000]
    for fn in ("bool estimateDisparity(", "int submitStereo("):
        assert "useLayout(" in src[src.index(fn):src.index(fn) + 2500], fn


def test_tf_broadcast_and_frames():
    src = open(NODE).read()
    assert 'ros::NodeHandle visual_odometry_nh(private_node_handle_, "visual_odometry")' in src
    assert 'param("base_link_frame_id", std::string("base_link"))' in src and 'param("odom_frame_id", std::string("odom"))' in src
    assert "tf_buffer_.canTransform(base_link_frame_id_, camera_frame_id_" in src
    assert "tf_buffer_.lookupTransform(base_link_frame_id_, camera_frame_id_" in src
    assert "impl_->odomToBase()" in src and "tf_broadcaster_.sendTransform(msg)" in src
    assert "msg.header.frame_id = odom_frame_id_" in src and "msg.child_frame_id = base_link_frame_id_" in src


def test_crop_parameters():
    src = open(NODE).read()
    assert 'param("crop_width", 0)' in src and 'param("crop_height", 0)' in src
    assert "mod_host::crop_camera_info(info, crop_width_, crop_height_)" in src
    assert "mod_host::centred_origin(" in src


def test_tf2_ros_in_both_manifests():
    doc = xml.dom.minidom.parse(os.path.join(PKG, "package.xml"))
    deps = {d.firstChild.data.strip() for tag in ("depend", "build_depend", "exec_depend") for d in doc.getElementsByTagName(tag)}
    assert "tf2_ros" in deps
    cm = open(os.path.join(PKG, "CMakeLists.txt")).read()
    comps = re.search(r"find_package\(catkin REQUIRED COMPONENTS(.*?)\)", cm, flags=re.S).group(1).split()
    assert "tf2_ros" in comps
