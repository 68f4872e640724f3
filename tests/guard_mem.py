"""Guarded host buffers for the bounds tests (tests/test_emu_bounds.py): every array lives in its own anonymous mapping with a
PROT_NONE page on either side, so a kernel run on the hipemu emulator that reads or writes one element outside the buffer it
was given faults at the statement that does it.  What the guard pages cannot see (the few bytes of slack that 16-byte alignment
leaves, the rest of the data pages) is filled with a canary; outputs are pre-filled with a NaN sentinel and `check()` verifies
that every element the API promises to write no longer holds it.

Placement "tail": the array ends as close to the upper guard page as a 16-byte aligned start allows (<= 15 bytes of slack, 12
for float32): an over-run faults.  Placement "head": the array starts right after the lower guard page: an under-run (row -1,
"the previous frame") faults.

``Banded`` is the device counterpart (tests/test_gpu_bounds.py): each buffer is a view into a larger torch tensor with sentinel
bands on either side; stray writes change the bands, stray reads of a band feed a NaN into the result."""
import ctypes
import mmap
import sys

import numpy as np

SENTINEL_F32 = 0x7FA5A5A5          # a quiet NaN with a payload no kernel computes
CANARY = 0xC3
PAGE = mmap.PAGESIZE
PROT_NONE, PROT_RW = 0, mmap.PROT_READ | mmap.PROT_WRITE

_libc = ctypes.CDLL(None, use_errno=True)
_libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
_libc.mprotect.restype = ctypes.c_int


def sentinel_bytes(dtype):
    """The sentinel pattern of one element: the NaN payload for float32, 0xA5 bytes for every other type."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.array([SENTINEL_F32], np.uint32).tobytes()
    return bytes([0xA5]) * dtype.itemsize


def sentinel_mask(a):
    """Elements of `a` that still hold the sentinel pattern, bit for bit."""
    a = np.ascontiguousarray(a)
    pat = np.frombuffer(sentinel_bytes(a.dtype), np.uint8)
    if a.size == 0:
        return np.zeros(a.shape, bool)
    raw = a.reshape(-1).view(np.uint8).reshape(a.size, a.dtype.itemsize)
    return np.all(raw == pat, axis=1).reshape(a.shape)


def fill_sentinel(a):
    a.reshape(-1).view(np.uint8)[:] = np.tile(np.frombuffer(sentinel_bytes(a.dtype), np.uint8), a.size)


class _Buf:
    def __init__(self, name, arr, placement, promised, lo, hi, canaries):
        self.name, self.arr, self.placement, self.promised = name, arr, placement, promised
        self.lo, self.hi = lo, hi                  # [start, end) of the array's bytes
        self.canaries = canaries                   # [(address, nbytes)] filled with CANARY


def _promised_mask(buf):
    p, a = buf.promised, buf.arr
    if p is None:
        return None
    if isinstance(p, str):
        assert p == "all", p
        return np.ones(a.shape, bool)
    if callable(p):
        return np.asarray(p(a), bool)
    return np.broadcast_to(np.asarray(p, bool), a.shape)


class Arena:
    """buf(name, shape, dtype, fill, placement, promised) -> numpy array in its own guarded mapping.

    fill: a scalar, an array (copied in) or "sentinel".  promised: None (an input or a workspace: nothing checked but the
    canaries), "all", a boolean mask broadcastable to the shape, or a callable(array) -> mask, evaluated at check() time."""

    def __init__(self, placement="tail", log=sys.stderr):
        assert placement in ("tail", "head")
        self.placement, self.log = placement, log
        self.bufs = []
        self._maps = []

    def buf(self, name, shape, dtype=np.float32, fill=0.0, placement=None, promised=None):
        placement = placement or self.placement
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape, dtype=np.int64))
        nbytes = n * dtype.itemsize
        rounded = (nbytes + 15) & ~15
        data_pages = max(1, (rounded + PAGE - 1) // PAGE)
        mm = mmap.mmap(-1, (data_pages + 2) * PAGE, flags=mmap.MAP_PRIVATE, prot=PROT_RW)
        base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
        data_lo, data_hi = base + PAGE, base + PAGE + data_pages * PAGE
        off = PAGE if placement == "head" else PAGE + data_pages * PAGE - rounded
        arr = np.frombuffer(mm, dtype=dtype, count=n, offset=off).reshape(shape)
        lo, hi = base + off, base + off + nbytes
        ctypes.memset(data_lo, CANARY, data_pages * PAGE)
        canaries = [(data_lo, lo - data_lo), (hi, data_hi - hi)]
        if isinstance(fill, str):
            assert fill == "sentinel", fill
            fill_sentinel(arr)
        elif isinstance(fill, np.ndarray):
            arr[...] = fill.reshape(shape)
        else:
            arr[...] = fill
        for addr in (base, data_hi):
            if _libc.mprotect(addr, PAGE, PROT_NONE) != 0:
                raise OSError(ctypes.get_errno(), "mprotect")
        self._maps.append(mm)
        self.bufs.append(_Buf(name, arr, placement, promised, lo, hi, canaries))
        return arr

    def describe(self, file=None):
        """The buffer map (name, [start, end), placement) to stderr: a fault address names its buffer and side."""
        f = file or self.log
        for b in self.bufs:
            print(f"guard_mem: {b.name:<24} [0x{b.lo:x}, 0x{b.hi:x}) {b.hi - b.lo:>10} B {b.placement}", file=f)
        f.flush()

    def problems(self):
        out = []
        for b in self.bufs:
            for addr, n in b.canaries:
                if n and ctypes.string_at(addr, n) != bytes([CANARY]) * n:
                    side = "below" if addr < b.lo else "above"
                    out.append(f"{b.name}: canary {side} the buffer overwritten")
            m = _promised_mask(b)
            if m is not None:
                left = sentinel_mask(b.arr) & m
                if left.any():
                    first = np.argwhere(left)[0].tolist()
                    out.append(f"{b.name}: {int(left.sum())} promised element(s) never written (first at {first})")
        return out

    def check(self):
        bad = self.problems()
        assert not bad, "; ".join(bad)

    # the allocator interface shared with Banded (tests/test_gpu_bounds.py)
    @staticmethod
    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)

    @staticmethod
    def get(a):
        return a

    def sync(self):
        pass


class Banded:
    """Device allocator: each buffer is a view into a larger uint8 torch tensor with bands of the sentinel on either side
    (>= 64 KiB, or the buffer's own size up to 16 MiB); the buffer's start is 256-byte aligned as torch's allocator gives."""

    def __init__(self, device="cuda", log=sys.stderr):
        import torch
        self.torch, self.device, self.log = torch, device, log
        self.bufs = []

    def buf(self, name, shape, dtype=np.float32, fill=0.0, placement=None, promised=None):
        torch = self.torch
        dtype = np.dtype(dtype)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = int(np.prod(shape, dtype=np.int64))
        nbytes = n * dtype.itemsize
        band = max(64 << 10, min(16 << 20, (nbytes + 255) & ~255))
        host = np.empty(band + ((nbytes + 255) & ~255) + band, np.uint8)
        host[:] = np.tile(np.frombuffer(sentinel_bytes(np.float32), np.uint8), host.size // 4)
        arr = host[band:band + nbytes].view(dtype).reshape(shape)
        if isinstance(fill, str):
            assert fill == "sentinel", fill
            fill_sentinel(arr)
        elif isinstance(fill, np.ndarray):
            arr[...] = fill.reshape(shape)
        else:
            arr[...] = fill
        whole = torch.from_numpy(host).to(self.device)
        view = whole[band:band + nbytes]
        self.bufs.append(dict(name=name, whole=whole, band=band, nbytes=nbytes, ref=host.copy(), dtype=dtype, shape=shape,
                              promised=promised, view=view))
        return view

    def describe(self, file=None):
        f = file or self.log
        for b in self.bufs:
            p = b["view"].data_ptr()
            print(f"guard_mem: {b['name']:<24} [0x{p:x}, 0x{p + b['nbytes']:x}) bands {b['band']} B", file=f)
        f.flush()

    def ptr(self, v):
        return None if v is None else ctypes.c_void_p(v.data_ptr())

    def get(self, v):
        for b in self.bufs:
            if b["view"] is v:
                return v.cpu().numpy().view(b["dtype"]).reshape(b["shape"])
        raise KeyError("not a buffer of this allocator")

    def sync(self):
        self.torch.cuda.synchronize()

    def problems(self):
        self.sync()
        out = []
        for b in self.bufs:
            whole = b["whole"].cpu().numpy()
            band, nb = b["band"], b["nbytes"]
            pad = (nb + 255) & ~255
            below, above = whole[:band], whole[band + nb:]
            if not np.array_equal(below, b["ref"][:band]):
                out.append(f"{b['name']}: band below the buffer changed")
            if not np.array_equal(above, b["ref"][band + nb:band + pad + band]):
                out.append(f"{b['name']}: band above the buffer changed")
            if b["promised"] is not None:
                arr = whole[band:band + nb].view(b["dtype"]).reshape(b["shape"])
                fake = _Buf(b["name"], arr, None, b["promised"], 0, 0, [])
                left = sentinel_mask(arr) & _promised_mask(fake)
                if left.any():
                    out.append(f"{b['name']}: {int(left.sum())} promised element(s) never written (first at {np.argwhere(left)[0].tolist()})")
        return out

    def check(self):
        bad = self.problems()
        assert not bad, "; ".join(bad)
