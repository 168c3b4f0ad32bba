"""`model.refine_net` (main/global_refine/model/refine_net.py:15): forwards to the gfx950 backend."""
from batrack_amd.global_refine import RefineNet  # noqa: F401
