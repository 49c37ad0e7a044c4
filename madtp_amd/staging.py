"""What the input paths share on the host: the pinned staging ring behind every batch's one host-to-device copy
(preprocess.ImagePipeline, jpeg.JpegDecoder, jpeg_device.DeviceJpegDecoder), align(), and the bounded thread pool of the decoders."""
import concurrent.futures
import threading

import torch

MAX_WORKERS = 16  # of any pool here; never sized from the machine's CPU count


def align(n, a):
    return (n + a - 1) // a * a


def grown(nbytes):
    """the size of a staging buffer made for a batch of nbytes: at least 1 MiB, a quarter above what was asked"""
    return max(nbytes, 1 << 20) * 5 // 4


class StagingRing:
    """Two pinned buffers used in turn, each guarded by an event: packing batch n + 1 does not wait for batch n, and a buffer is
    rewritten only after the copy that last read it has finished."""

    def __init__(self):
        self._stage = [None, None]
        self._events = [None, None]
        self._turn = 0

    def _next(self, nbytes):
        """-> (the turn taken, the size its buffer must be made with, or 0 if the one it has holds nbytes)"""
        i = self._turn
        self._turn ^= 1
        have = 0 if self._stage[i] is None else self._stage[i].numel()
        return i, 0 if nbytes <= have else grown(nbytes)

    def acquire(self, nbytes):
        """-> (turn, the next pinned buffer as a uint8 tensor of at least nbytes), once the copy that last read it has finished"""
        i, make = self._next(nbytes)
        if self._events[i] is not None:
            self._events[i].synchronize()
        if make:
            self._stage[i] = torch.empty(make, dtype=torch.uint8, pin_memory=True)
        return i, self._stage[i]

    def sent(self, turn):
        """after the copy out of buffer `turn` was enqueued: records its event on the current stream"""
        if self._events[turn] is None:
            self._events[turn] = torch.cuda.Event()
        self._events[turn].record()


class Pool:
    """map() over at most MAX_WORKERS threads, made on first use (ctypes releases the GIL in the library's host calls)"""

    def __init__(self, workers, name):
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self._name = name
        self._pool = None

    def map(self, fn, jobs):
        if self.workers == 1 or len(jobs) < 2:
            return [fn(j) for j in jobs]
        if self._pool is None:
            self._pool = concurrent.futures.ThreadPoolExecutor(self.workers, thread_name_prefix=self._name)
        futures = [self._pool.submit(fn, j) for j in jobs]
        concurrent.futures.wait(futures)  # all of them: a failed batch leaves no thread writing into the staging buffer
        return [f.result() for f in futures]


class StatusWaiter:
    """The wait for a launch's status words: copied on a side stream, behind an event recorded after the kernel, into a pinned
    buffer; only that stream is synchronised."""

    def __init__(self):
        self._lock = threading.Lock()
        self._side, self._host = {}, None

    def read(self, status):
        dev, n = status.device, status.numel()
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        with self._lock:
            side = self._side.get(dev)
            if side is None:
                side = self._side[dev] = torch.cuda.Stream(device=dev)
            if self._host is None or self._host.numel() < n:
                self._host = torch.empty(max(n, 256), dtype=torch.int32, pin_memory=True)
            side.wait_event(done)
            status.record_stream(side)
            with torch.cuda.stream(side):
                self._host[:n].copy_(status, non_blocking=True)
            side.synchronize()
            return self._host[:n].numpy().copy()
