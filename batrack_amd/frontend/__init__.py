"""What batrack_amd provides of the reference's tracker front end (main/frontend): the correlation lookup.

  batrack_amd.frontend.corr.CorrBlock     the tracker's CorrBlock, fused: no correlation volume
  batrack_amd.frontend.corr.install       make the reference's unmodified md_tracker use it
"""
