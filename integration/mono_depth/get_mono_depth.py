"""`main/mono_depth/get_mono_depth.py` (the numeric step of scripts/demo/run_mono_depth.sh) over batrack_amd.mono_depth:
`intrinsics_to_fov`, `align_depth` and `align_davis_demo` with the reference's signatures, the alignment on the GPU
(bt_mono_align, include/batrack_depth.h).  Run as the reference is run:

    python integration/mono_depth/get_mono_depth.py --depth_dir DIR --data_dir DIR [--save_name NAME]
"""
import argparse
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if _ROOT not in sys.path:
    sys.path.append(_ROOT)                                   # run as a script: the repository's package

from batrack_amd.mono_depth import align_davis_demo, align_depth, intrinsics_to_fov  # noqa: E402,F401

if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="Align monocular and metric depth maps")
    parser.add_argument("--depth_dir", type=str, required=True, help="Directory containing depth estimations")
    parser.add_argument("--data_dir", type=str, required=True, help="Directory containing input images")
    parser.add_argument("--save_name", type=str, default="unidepth_da", help="Name for the saved directory")
    args = parser.parse_args()
    align_davis_demo(args.depth_dir, args.data_dir, args.save_name)
