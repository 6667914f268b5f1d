"""GPU: crop decode (dwtx_decode_view_crop) swept over origins, crop sizes and thin shapes — the edge arithmetic of
k_inv_level_roi (lift.hip, section "crop decode") held to the oracle.

tests/test_crop_gpu.py covers the call's sinks, sample types and refusals at some 40 (shape, size, origin) points.  Here the
sink is the plainest there is — uint8, dense windows — and the points are many: one noise picture per shape, encoded by the
oracle once, its stream repeated in up to 512 rows (four decoder parts, each with its slice of the origin table), every row
with an origin of its own.  After each call the WHOLE buffer must equal the oracle's picture sliced once per row
(sliding_window_view, no loop).  Every comparison is exact; no origin is left out.

The cases are tests/crop.py's sweep_groups(); tests/test_crop_sweep_cpu.py derives from the restated host arithmetic which
parities, clamped origins, strip counts, frozen samples and band-sized rectangles they reach at every windowed level."""
import numpy as np
import pytest

import crop
import levels
import test_float_gpu as F
import test_views_gpu as V

pytestmark = pytest.mark.gpu

GROUPS = crop.sweep_groups()


def picture_key(c):
    return (c.W, c.H, c.Cn, c.reduced)


ROWS = {}   # picture -> the most rows a call of its cases has
for _cases in GROUPS.values():
    for _c in _cases:
        ROWS[picture_key(_c)] = max(ROWS.get(picture_key(_c), 0), min(len(_c.origins), crop.CALL_MAX))


@pytest.fixture(scope="module")
def uploaded(ctx):
    """case -> (streams, lens, the oracle's picture): the shape's one stream in as many rows as its largest call has, uploaded
    once and dropped with the module"""
    held = {}

    def get(c):
        key = picture_key(c)
        if key not in held:
            data, pic = crop.sweep_stream(c)
            held[key] = F.upload(ctx, [data] * ROWS[key]) + (pic,)
        return held[key]

    yield get
    held.clear()


def dense(n, cw, ch, Cn):
    return V.Layout(n * ch * cw * Cn, 0, (n, ch, cw, Cn), (ch * cw * Cn, cw * Cn, Cn, 1))


def expectation(pic, buf, org, cw, ch):
    """buf [n, ch, cw, C], prefilled: row i receives pic[y0:y0 + ch, x0:x0 + cw], as far as the picture reaches"""
    oh, ow = pic.shape[:2]
    inside = (org[:, 0] + cw <= ow) & (org[:, 1] + ch <= oh)
    if cw <= ow and ch <= oh:
        win = np.lib.stride_tricks.sliding_window_view(pic, (ch, cw), axis=(0, 1))   # [y0, x0, C, ch, cw]
        buf[inside] = win[org[inside, 1], org[inside, 0]].transpose(0, 2, 3, 1)
    for i in np.flatnonzero(~inside):   # (reduced pictures only: a crop across the edge is clipped, one beyond it leaves its window alone)
        part = pic[org[i, 1]:org[i, 1] + ch, org[i, 0]:org[i, 0] + cw]
        buf[i, :part.shape[0], :part.shape[1]] = part


def run_case(ctx, opts, uploaded, c):
    streams, lens, pic = uploaded(c)
    W, H = c.reduced or (c.W, c.H)
    opts.set("crop_route", c.route)
    opts.set("lift_rows", c.rows_per_wave)
    level = levels.levels_of(W, H) - (2 if c.reduced else 1)
    for first in range(0, len(c.origins), crop.CALL_MAX):
        org = np.array(c.origins[first:first + crop.CALL_MAX])
        n = len(org)
        L = dense(n, c.cw, c.ch, c.Cn)
        buf = V.pattern(L.samples, False)
        want = buf.copy()
        expectation(pic, want.reshape(L.shape), org, c.cw, c.ch)
        tbuf = V.to_device(ctx, buf)
        infos = ctx.decode_view_crop(streams[:n], lens[:n], L.t_view(tbuf), (W, H), [(int(x), int(y)) for x, y in org])
        assert all(I.status == 0 and I.level == level for I in infos)
        got = V.to_host(tbuf, False)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i, y, x, k = np.unravel_index(bad, L.shape)
            rows = np.unique(i)
            raise AssertionError(
                f"{W}x{H}x{c.Cn}, crop {c.cw}x{c.ch}, route {c.route}, lift_rows {c.rows_per_wave}: {bad.size} samples differ in {rows.size} of {n} "
                f"windows; origins {org[rows[:8]].tolist()}; first at origin {org[i[0]].tolist()} row {y[0]} column {x[0]} channel {k[0]}: "
                f"got {got[bad[0]]}, want {want[bad[0]]}")


@pytest.mark.parametrize("name", list(GROUPS))
def test_crop_sweep(ctx, opts, uploaded, name):
    for c in GROUPS[name]:
        run_case(ctx, opts, uploaded, c)
