"""Pinned staging buffers and the copy thread pool of the block loader (FlatIPIndex.add of a host array), on the GPU's NUMA node.
They are process-wide: pinning 64 MB costs ~20 ms (hipHostMalloc), i.e. a fresh set per index would cost as much as loading a
3 GB block through them."""
import os
import threading

from . import _lib

_STAGING = {}
_STAGING_THREADS = {}
_POOLS = {}
_STAGING_LOCK = threading.Lock()         # guards the dictionaries
_STAGING_BUILD = threading.Lock()        # held while buffers are allocated and pinned
_NUMA = {}


def gpu_numa_cpus(device):
    """CPUs of the NUMA node the GPU hangs off (None when the topology cannot be read, or on a one-node host).
    A pinned buffer is placed where its allocating thread runs; across the socket link the same H2D copy runs at 29 GB/s
    instead of 57 (measured on a 2-socket MI355X host, tools/dbg/loader_probe.py) -- which is why the loader's rate, and the
    'pinned H2D ceiling' beside it, used to differ by a factor of two between boxes of one pool."""
    import torch
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _NUMA:
        return _NUMA[idx]
    cpus = None
    try:
        import ctypes
        buf = ctypes.create_string_buffer(64)
        # (through libconvdr_hip.so, which is bound to the HIP runtime torch loaded: dlopen-ing "libamdhip64.so" by name
        #  brings a SECOND runtime into the process, which slowed every later launch -- the training step went host-bound)
        if _lib.lib().convdr_device_pci_bus_id(int(idx), buf, 64) == 0:
            bdf = buf.value.decode().lower()
            node = int(open("/sys/bus/pci/devices/%s/numa_node" % bdf).read().strip())
            import glob
            if node >= 0 and len(glob.glob("/sys/devices/system/node/node[0-9]*")) > 1:
                got = set()
                for part in open("/sys/devices/system/node/node%d/cpulist" % node).read().strip().split(","):
                    lo, _, hi = part.partition("-")
                    got.update(range(int(lo), int(hi or lo) + 1))
                got &= os.sched_getaffinity(0)
                cpus = got or None
    except Exception:
        cpus = None
    _NUMA[idx] = cpus
    return cpus


class _on_cpus:
    """Confine the calling thread to `cpus` for the duration of the block (no-op for None)."""

    def __init__(self, cpus):
        self.cpus, self.old = cpus, None

    def __enter__(self):
        if self.cpus:
            try:
                self.old = os.sched_getaffinity(0)
                os.sched_setaffinity(0, self.cpus)
            except OSError:
                self.old = None

    def __exit__(self, *exc):
        if self.old is not None:
            os.sched_setaffinity(0, self.old)


def pinned_near(device, shape, dtype):
    """A pinned host tensor allocated (first-touched and locked) on the GPU's NUMA node."""
    import torch
    with _on_cpus(gpu_numa_cpus(device)):
        t = torch.empty(shape, dtype=dtype).pin_memory()
    return t


def _staging_key(device, d, nbuf):
    return (str(device), int(d), int(nbuf))


def _staging(device, rows, d, nbuf):
    """([nbuf pinned [rows, d] fp32 buffers], [their last H2D-copy events]) of `device`: process-wide, grown on demand.
    Serialised by _STAGING_BUILD (a background pre-pin -- FlatIPIndex.prepin_staging -- and the first add() may race)."""
    import torch
    key = _staging_key(device, d, nbuf)
    with _STAGING_BUILD:
        ent = _STAGING.get(key)
        if ent is None or ent[0][0].shape[0] < rows:
            ent = ([pinned_near(device, (rows, d), torch.float32) for _ in range(nbuf)], [None] * nbuf)
            with _STAGING_LOCK:
                _STAGING[key] = ent
    return ent


def _copy_pool(threads, device=None):
    """Reader threads of the block loader; confined to the GPU's NUMA node (their destination is the pinned staging there)."""
    cpus = gpu_numa_cpus(device) if device is not None else None
    key = (threads, None if cpus is None else min(cpus))
    pool = _POOLS.get(key)
    if pool is None:
        from concurrent.futures import ThreadPoolExecutor

        def init():
            if cpus:
                try:
                    os.sched_setaffinity(0, cpus)
                except OSError:
                    pass
        pool = _POOLS[key] = ThreadPoolExecutor(max_workers=threads, initializer=init)
    return pool
