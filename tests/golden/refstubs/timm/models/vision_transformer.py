"""Empty stand-in: the reference's cotracker/blocks.py imports these two names; the fixture generators never call them."""


class Attention:
    pass


class Mlp:
    pass
