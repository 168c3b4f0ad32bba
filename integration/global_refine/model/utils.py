"""`model.utils` (main/global_refine/model/utils.py:103-116, 203-265): the depth evaluation, forwarded."""
from batrack_amd.evaluation import compute_errors, eval_depth, eval_depth_metric, print_results  # noqa: F401
