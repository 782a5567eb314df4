"""CPU: the member-list ABI (mod_set_cluster_members / mod_get_cluster_members) — struct size, exports, what the header promises,
and where the kernel lives in the source."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mod_sf.h")
CSRC = os.path.join(ROOT, "moving_object_detector_amd", "csrc")


def test_struct_is_32_bytes_and_mirrors_the_header():
    from moving_object_detector_amd import capi
    assert C.sizeof(capi.ModClusterMembers) == 32
    assert [n for n, _ in capi.ModClusterMembers._fields_] == ["offsets", "indices", "points", "reserved"]
    assert capi.ModClusterMembers.reserved.offset == 24 and capi.ModClusterMembers.reserved.size == 8
    src = open(HEADER).read()
    body = re.search(r"typedef struct ModClusterMembers \{(.*?)\} ModClusterMembers;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*;", body) == ["offsets", "indices", "points", "reserved"]


def test_both_symbols_are_exported_and_bound():
    from moving_object_detector_amd import capi
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("mod_set_cluster_members", "mod_get_cluster_members"):
        assert name in names and name in capi.EXPORTS
    lib = capi.load()
    assert lib.mod_set_cluster_members.argtypes[1]._type_ is capi.ModClusterMembers
    # a NULL context is refused before anything else, like every other setter
    assert lib.mod_set_cluster_members(None, None) == capi.MOD_ERR_INVALID_ARGUMENT
    assert lib.mod_get_cluster_members(None, None, None) == capi.MOD_ERR_INVALID_ARGUMENT


def test_header_states_the_order_and_the_submit_rule():
    src = " ".join(re.sub(r"\n \*(?!/)", "\n", open(HEADER).read()).split())     # one line, without the comments' leading " *"
    doc = src[src.index("Per-cluster member lists"):src.index("typedef struct ModClusterMembers")]
    assert "u ascending, then v ascending" in doc and "v * W + u" in doc
    assert "mod_submit_*_host calls never write the lists" in doc
    assert "mod_process_frame_host and mod_cluster_cloud_host, as frame 0" in doc
    assert "at and beyond offsets[f][K] are not written" in doc
    assert "NULL = off" in doc and "reserved != 0" in doc
    # the ABI around it is unchanged
    assert "#define MOD_STAGE_COUNT 7" in src and "#define MOD_PROFILE_ALL 0x7f" in src
    from moving_object_detector_amd import capi
    assert C.sizeof(capi.ModClusterOut) == 32


def test_the_kernel_sits_between_the_final_and_the_median_launch_and_shares_the_layout():
    host = open(os.path.join(CSRC, "mod_sf.hip")).read()
    i, j, k = host.index("launch_final(c->dc"), host.index("launch_cluster_members(c->dc"), host.index("launch_median(c->dc")
    assert i < j < k
    assert re.search(r"if \(mem\) launch_cluster_members", host), "no launch while the setting is off"
    common = open(os.path.join(CSRC, "cluster_common.h")).read()
    assert common.count("int member_layout(") == 1 and "tie_row_col" in common
    for name in ("cluster_median.hip", "cluster_final.hip"):       # both kernels call the one device function
        assert "member_layout<" in open(os.path.join(CSRC, name)).read(), name
    # the pipelined submits hand the cluster stage no lists
    api = open(os.path.join(CSRC, "host_api.hip")).read()
    assert "process_dev(c, &in, &pl, &out, nullptr)" in api
