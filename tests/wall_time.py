"""A test's wall time, printed once (pytest -s, or the captured output of a failure, shows it)."""
import time


class wall:
    """with wall("name"): ... -- the block's wall time, printed once"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        print("wall time of %s: %.2f s" % (self.name, time.perf_counter() - self.t0))
