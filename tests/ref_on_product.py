"""TEST INFRASTRUCTURE: the two "reference sources, unchanged, on top of the product" artefacts, built by oracle/Makefile
(`make on_product`) into oracle/_ref/ beside the other reference builds.  Used by tests/conftest.py and by
__graft_entry__.build(); they need /root/reference, so they are built where its sources exist and found prebuilt elsewhere."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SRC = "/root/reference/surfel_fusion/src"
ORACLE = os.path.join(ROOT, "oracle")
ROS_NODE_ON_PRODUCT = os.path.join(ORACLE, "_ref", "ros_node_on_product")
REF_MAP_ON_PRODUCT = os.path.join(ORACLE, "_ref", "libdsm_ref_map_on_product.so")


def _make(out):
    from densesurfelmapping_amd import build
    build.build_library()
    subprocess.run(["make", "-s", "-C", ORACLE, out], check=True, stdout=subprocess.DEVNULL)
    return out


def build_ros_node_on_product():
    """surfel_fusion/src/ros_node.cpp, in place and unchanged, against include/ros_compat."""
    return _make(ROS_NODE_ON_PRODUCT)


def build_ref_map_on_product():
    """surfel_fusion/src/surfel_map.{h,cpp}, in place and unchanged, with FusionFunctions = the product's facade
    (include/engine_compat), behind the C driver of oracle/ref_map_driver.cpp."""
    return _make(REF_MAP_ON_PRODUCT)
