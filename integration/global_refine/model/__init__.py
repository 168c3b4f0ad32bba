"""`model` of the reference's main/global_refine, served by batrack_amd (integration/README.md)."""
