"""What MapfGridBatch, MarlPartialBatch and PrimalBatch share over the C ABI.

Pure argument handling first (NumPy arrays and CPU tensors work, so it is tested
without a GPU): seeds, [E, N, 2] agent arrays, grids / bitmaps, on-grid checks,
action and env-mask coercion.  Then `DeviceBatch`, the base of the three batches:
the device, the handle's lifetime, the launch path, allocation (plain or packed
into one flat buffer) and the invalid-action report.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ._abi import MAPFX_I8, MAPFX_I32, MAPFX_I64, check
from .maps import map_stride, pack_bits

DTYPES = {torch.int8: MAPFX_I8, torch.int32: MAPFX_I32, torch.int64: MAPFX_I64}


def u64(seed) -> int:
    """A Python int as the C ABI's uint64 seed (two's complement of a negative one)."""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def parse_agents(a, b, names):
    """Two [E, N, 2] (row, col) arrays -> (E, N, a int32, b int32)."""
    a, b = np.array(a, dtype=np.int32), np.array(b, dtype=np.int32)
    if a.ndim != 3 or a.shape[-1] != 2 or b.shape != a.shape:
        raise ValueError("%s must both be [E, N, 2]" % names)
    return int(a.shape[0]), int(a.shape[1]), a, b


def parse_map(grids, bits, hw, E, obstacle=lambda g: g != 0):
    """`grids` [H, W] or [E|1, H, W] (packed where obstacle(grids) holds), or ready-made
    `bits` [E|1, map_stride] with hw = (H, W) -> (H, W, bits uint8 [E|1, stride],
    map_shared: one map for more than one env)."""
    if bits is None:
        g = np.asarray(grids)
        if g.ndim == 2:
            g = g[None]
        H, W = int(g.shape[1]), int(g.shape[2])
        bits = pack_bits(obstacle(g))
    else:
        H, W = hw
    bits = np.array(bits, dtype=np.uint8)
    if bits.ndim == 1:
        bits = bits[None]
    if bits.shape[1] != map_stride(H, W) or bits.shape[0] not in (1, E):
        raise ValueError("bits must be [E or 1, %d]" % map_stride(H, W))
    return H, W, bits, bits.shape[0] == 1 and E != 1


def check_on_grid(arr, H, W, what):
    """ValueError unless every (row, col) of arr [..., 2] lies in [0, H) x [0, W): the
    kernels index their cell maps with them."""
    if arr.size and (arr[..., 0].min() < 0 or arr[..., 0].max() >= H
                     or arr[..., 1].min() < 0 or arr[..., 1].max() >= W):
        raise ValueError("%s outside the %dx%d grid" % (what, H, W))


def as_actions(a, device, shape=None):
    """Actions -> (contiguous int8 / int32 / int64 tensor on `device`, its MAPFX_I* code);
    any other dtype becomes int64.  A tensor that already is all that is returned as it
    is, at the cost of no torch call.  `shape` None: the caller checks the shape."""
    if not (isinstance(a, torch.Tensor) and a.device == device and a.dtype in DTYPES
            and a.is_contiguous()):
        a = torch.as_tensor(a, device=device)
        if a.dtype not in DTYPES:
            a = a.to(torch.int64)
        a = a.contiguous()
    if shape is not None and a.shape != shape:
        raise AssertionError("actions must be %s, got %s" % (list(shape), list(a.shape)))
    return a, DTYPES[a.dtype]


def env_mask(mask, E, device):
    """An env mask -> uint8 [E] on `device` (None stays None): uint8 as it is, any other
    dtype by `!= 0`.  The kernels read E bytes of it, so any other shape is refused."""
    if mask is None:
        return None
    m = torch.as_tensor(mask, device=device)
    if m.shape != (E,):
        raise AssertionError("mask must be [E] (E = %d), got %s" % (E, list(m.shape)))
    return (m if m.dtype == torch.uint8 else (m != 0).to(torch.uint8)).contiguous()


def avail_bits(mask):
    """[...] 5-bit available-action masks -> [..., 5] int64 0/1 (get_avail_actions)."""
    bits = torch.arange(5, device=mask.device, dtype=torch.uint8)
    return ((mask.unsqueeze(-1) >> bits) & 1).to(torch.int64)


class DeviceBatch:
    """E envs behind one C-ABI handle on one HIP device."""

    packed = False              # _alloc_spec(..., packed=True): one flat buffer
    _layout = _flat = None

    def __init__(self, device):
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda":
            raise RuntimeError("%s runs on a HIP device only (got %s)"
                               % (type(self).__name__, self.device))

    def _create(self, create, destroy, cfg):
        """self._h = create(cfg) on self.device; __del__ hands it to `destroy`."""
        with torch.cuda.device(self.device):
            h = ctypes.c_void_p()
            check(create(ctypes.byref(cfg), ctypes.byref(h)), create.__name__)
        self._h, self._destroy = h, destroy
        self._dev_index = self.device.index if self.device.index is not None \
            else torch.cuda.current_device()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._destroy(h)
            self._h = None

    def _call(self, fn, *args):
        """Run a C-ABI call with self.device current (no context switch when it already is)."""
        if torch.cuda.current_device() == self._dev_index:
            return fn(*args, torch.cuda.current_stream().cuda_stream)
        with torch.cuda.device(self.device):
            return fn(*args, torch.cuda.current_stream().cuda_stream)

    def _zeros(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def _zeros_of(self, spec):
        return {k: self._zeros(shape, dt) for k, (shape, dt) in spec.items()}

    def _alloc_spec(self, spec, packed):
        """name -> zeroed tensor of a name -> (shape, dtype) spec.  `packed`: all of them
        are views of ONE flat device buffer (mapfx.dist.ChunkLayout), so a host mirror of
        everything a drop-in env reads after a step is a single copy."""
        self.packed = bool(packed)
        if not self.packed:
            return self._zeros_of(spec)
        from .dist import ChunkLayout
        self._layout = ChunkLayout(spec)
        self._flat = self._layout.alloc(self.device)
        return self._layout.views(self._flat)

    def host_mirror(self):
        """Pinned host copy of the packed buffer and its typed views (packed=True)."""
        if not self.packed:
            raise RuntimeError("host_mirror needs %s(..., packed=True)" % type(self).__name__)
        flat = torch.empty(self._layout.nbytes, dtype=torch.uint8, pin_memory=True)
        return flat, self._layout.views(flat)

    def pull(self, host_flat):
        """Copy the packed buffer (state + outputs) into `host_flat` (host_mirror) and
        wait for it: the one synchronisation of a drop-in step."""
        host_flat.copy_(self._flat, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return host_flat

    def _take_err(self, err):
        """1 + the env a kernel reported in `err` since the last call, or 0; clears it
        (synchronises)."""
        e = int(err.item())
        if e:
            err.zero_()
        return e

    def check_err(self):
        """Raise AssertionError like the reference if an env got an action outside
        0..4 since the last call (synchronises)."""
        e = self._take_err(self.err)
        if e:
            raise AssertionError("invalid action for env %d (actions must be in 0..4)" % (e - 1))
