"""Flips in views (the *_view_flip calls, include/dwtx.h) — test infrastructure only, CPU only: the contract restated with
numpy, which does take negative strides.

A window's flags are a mask: X = 1 mirrors the columns, Y = 2 the rows.  Memory position (x, y) of a window of Ww x Hw
holds pixel (u, v) of the window's picture with u = Ww - 1 - x under X and v = Hw - 1 - y under Y.  Arrays are [H, W, ...]."""
import numpy as np

X, Y = 1, 2
FLAGS = (0, 1, 2, 3)
MIXED = [0, 1, 2, 3, 1]   # the per-picture list of five windows


def in_memory(pic, f):
    """The picture as it lies in a window with flags f — and, the same operation, the picture a window with flags f holds.
    A view of `pic`: writing to it writes the picture."""
    assert f in FLAGS
    if f & X:
        pic = pic[:, ::-1]
    if f & Y:
        pic = pic[::-1]
    return pic


def place(window, part, f):
    """Write `part`, a picture that came out no larger than its window (a reduced picture, a crop's part inside one), into
    `window` (memory order) as a call with flags f leaves it: in the corner where the window's pixel (0, 0) lies — under Y the
    bottom rows, under X the right-hand columns — and nothing else of the window."""
    h, w = part.shape[:2]
    assert h <= window.shape[0] and w <= window.shape[1]
    in_memory(window, f)[:h, :w] = part


def walked(buf, origin, pitch, step, cs, H, W, C):
    """The picture the table of dwtx_view_flip_plan walks: pixel (u, v)'s channel c at buf[origin + v * pitch + u * step + c * cs],
    signed strides and all, as a strided view of the flat sample buffer."""
    k = buf.itemsize
    lo = origin + min(0, (H - 1) * pitch) + min(0, (W - 1) * step)
    hi = origin + max(0, (H - 1) * pitch) + max(0, (W - 1) * step) + (C - 1) * cs
    assert 0 <= lo and hi < buf.size, (lo, hi, buf.size)
    return np.lib.stride_tricks.as_strided(buf[origin:], (H, W, C), (pitch * k, step * k, cs * k))
