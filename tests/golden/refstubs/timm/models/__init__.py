"""Empty stand-in: the reference's cotracker/blocks.py imports the name; the fixture generators never call it."""
