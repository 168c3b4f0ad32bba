"""Stand-in for `timm` that tests/golden/make_golden_update_former.py puts first on sys.path: see models/vision_transformer.py."""
