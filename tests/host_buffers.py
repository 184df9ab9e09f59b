"""TEST INFRASTRUCTURE (numpy and ctypes only: the emulated and the GPU suites both import it).  Host arrays as the C ABI
takes them: `ptr`; outputs between guard bands: `Guarded`; the comparisons of two arrays that are rules of no one kernel:
`same_bits`, `compare_bits`, `relative_difference`."""
import ctypes as C

import numpy as np

GUARD = 64          # elements of 0xA5 bytes on either side of every output


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)  # (the pointer object keeps the array alive)


class Guarded:
    """name -> poisoned array between two guard bands"""

    def __init__(self, shapes):
        self.raw, self.view = {}, {}
        for k, (shape, dt) in shapes.items():
            n = int(np.prod(shape))
            raw = np.full((n + 2 * GUARD) * np.dtype(dt).itemsize, 0xA5, np.uint8)
            v = raw.view(dt)[GUARD:GUARD + n].reshape(shape)
            v[...] = np.nan if np.issubdtype(dt, np.floating) else 0x55
            self.raw[k], self.view[k] = raw, v

    def ptr(self, k):
        return self.view[k].ctypes.data if self.view[k].size else self.raw[k].ctypes.data + GUARD * self.view[k].dtype.itemsize

    def guards_intact(self):
        for k, raw in self.raw.items():
            g = GUARD * self.view[k].dtype.itemsize
            assert (raw[:g] == 0xA5).all() and (raw[len(raw) - g:] == 0xA5).all(), k
        return True

    def untouched(self):
        return all(np.isnan(v).all() if np.issubdtype(v.dtype, np.floating) else (v == 0x55).all() for v in self.view.values())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def compare_bits(got, want, what=""):
    for k, w in want.items():
        g = np.asarray(got[k])
        assert same_bits(g, np.asarray(w, g.dtype).reshape(g.shape)), (what, k)


def relative_difference(got, want):
    """the largest |got - want| / max(|want|, tiny) over the elements; equal bits (NaN and infinities included) count as 0"""
    g, w = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    same = (g == w) | (np.isnan(g) & np.isnan(w))
    if same.all():
        return 0.0
    with np.errstate(all="ignore"):
        d = np.abs(g - w) / np.maximum(np.abs(w), np.finfo(np.float64).tiny)
    d = np.where(same, 0.0, d)
    return float(np.inf if np.isnan(d).any() else d.max())
