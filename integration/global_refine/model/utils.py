"""`model.utils` (main/global_refine/model/utils.py:103-116, 203-312): the depth evaluation and the depth-map alignment,
forwarded."""
from batrack_amd.evaluation import compute_errors, eval_depth, eval_depth_metric, print_results  # noqa: F401
from batrack_amd.global_refine import align_depth_maps  # noqa: F401
