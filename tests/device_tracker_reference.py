"""A numpy statement of the tracker's state machine on the device (include/elo.h, elo_model_begin / elo_model_advance) for
tests/test_device_tracker_gpu.py, vetted on the CPU by tests/test_device_tracker_cpu.py against a plain list of "the last K scans".

State: {next in 0 .. K-1, held in 0 .. K}.  begin: where held == 0, frame 2 enters slot 0.  advance: (next', held') = held == 0 ?
(1 % K, 1) : (next, held); the scan enters slot next'; every pose row is re-based, row next' becomes the identity; state <-
{(next' + 1) % K, min(held' + 1, K)}."""
import numpy as np

import local_model_reference as M

IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0])


def entry(next_, held, K):
    """(next', held'): the slot the scan of an advance enters and the count it finds."""
    return (1 % K, 1) if held == 0 else (next_, held)


def after(next_, held, K):
    """The state an advance leaves."""
    n, h = entry(next_, held, K)
    return (n + 1) % K, min(h + 1, K)


class Machine:
    """The four state arrays of one tracker, moved by begin() / advance() as the launches move them.  `ring` holds whatever a
    caller enters: images (K,H,W,3) or, with shape=(), one scan number per slot."""

    def __init__(self, K, shape=(), dtype=np.float32, empty=0):
        self.K, self.empty = K, empty
        self.ring = np.full((K,) + tuple(shape), empty, dtype)
        self.poses64 = np.tile(IDENTITY, (K, 1))
        self.state = (0, 0)

    def reset(self):
        self.ring[...] = self.empty
        self.poses64[...] = IDENTITY
        self.state = (0, 0)

    def begin(self, first):
        if self.state[1] == 0:
            self.ring[0] = first

    def advance(self, scan, T=IDENTITY):
        slot, _held = entry(*self.state, self.K)
        self.ring[slot] = scan
        self.poses64[...] = M.rebase(self.poses64, T)
        self.poses64[slot] = IDENTITY
        self.state = after(*self.state, self.K)
        return slot

    def step(self, scan, first, T=IDENTITY):
        self.begin(first)
        return self.advance(scan, T)
