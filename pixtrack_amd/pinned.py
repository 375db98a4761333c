"""The two pinned-memory mechanisms of the host path, once each: a ring of blocks whose raw pointers kernels write to,
and the staging of a frame's 16-bit sensor depth image."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch


class PinnedRing:
    """``n`` zeroed pinned blocks of one shape, allocated on first use and handed out round-robin.

    A kernel that writes a record for the host receives the block's raw pointer, so torch's host allocator cannot know
    when the block is free again: the blocks therefore live as long as the ring's owner (a testbed, a refiner, a
    tracker, a lock-step group).  ``n = 8`` suffices: an owner takes at most two blocks per frame, and a frame's kernels
    have finished - its LM result was read, its records decoded in that frame's policy - long before eight more hand-outs
    are queued.  What is cleared on hand-out is the caller's business (a whole record, one column, nothing)."""

    def __init__(self, shape, dtype, n: int = 8):
        self.shape, self.dtype, self.n = tuple(int(x) for x in shape), dtype, int(n)
        self._blocks: Optional[list] = None
        self._next = 0

    def next(self, rows: Optional[int] = None) -> torch.Tensor:
        """The next block; ``rows``: its first ``rows`` rows.  More rows than the blocks have: every block is allocated
        anew with that many (the old ones stay alive with whoever still holds them)."""
        grow = rows is not None and rows > self.shape[0]
        if grow:
            self.shape = (int(rows),) + self.shape[1:]
        if self._blocks is None or grow:
            self._blocks = [torch.zeros(self.shape, dtype=self.dtype).pin_memory() for _ in range(self.n)]
        block = self._blocks[self._next]
        self._next = (self._next + 1) % self.n
        return block if rows is None else block[:rows]


class SensorStage:
    """One sensor depth image on its way to the device: a pinned buffer, a device buffer and the event of the last
    upload, all three living as long as their owner and re-allocated only when the image's shape changes."""

    def __init__(self, device):
        self.device = device
        self.host = self.dev = self.uploaded = None

    def upload(self, sensor, frame_name) -> torch.Tensor:
        """Queues the upload of ``sensor`` (uint16 [H, W]; ValueError otherwise) on the current stream and returns the
        device buffer, int16 with the same 16-bit patterns.  Nothing is awaited but the previous upload from the same
        pinned buffer."""
        sensor = np.ascontiguousarray(np.asarray(sensor))
        if sensor.dtype != np.uint16 or sensor.ndim != 2:
            raise ValueError(f"the sensor depth image of {frame_name} is {sensor.dtype} {sensor.shape}, not uint16 [H, W]")
        if self.host is None or tuple(self.host.shape) != sensor.shape:
            self.host = torch.empty(sensor.shape, dtype=torch.int16).pin_memory()
            self.dev = torch.empty(sensor.shape, dtype=torch.int16, device=self.device)
            self.uploaded = torch.cuda.Event()
        else:
            self.uploaded.synchronize()  # (the last frame's upload: over long ago, unless that frame ended early)
        self.host.numpy()[...] = sensor.view(np.int16)
        self.dev.copy_(self.host, non_blocking=True)
        self.uploaded.record(torch.cuda.current_stream(self.device))
        return self.dev
