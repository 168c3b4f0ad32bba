"""`model.trainer` (main/global_refine/model/trainer.py:5-77): forwards."""
from batrack_amd.global_refine import (adjust_learning_rate_by_lr, cosine_schedule, global_alignment_iter,  # noqa: F401
                                       global_alignment_loop, linear_schedule)
