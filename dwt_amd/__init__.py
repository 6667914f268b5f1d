"""dwt_amd — host-side mirror of the xdsopl/dwt encode/decode hot path on MI355X.

Everything here is plumbing over the C ABI in include/dwtx.h (libdwtx.so,
hand-written HIP for gfx950): torch supplies device memory and streams, the
library does the work.  Function names follow the reference's
(`transformation`, `linearization`, `reconstruction`, ... in encode.c/decode.c).
There is no CPU fallback: without the built library or without a GPU the calls
raise.
"""
import ctypes as C

from . import _lib
from ._lib import Geom, Stats, StreamInfo, DecodeInfo, Index, SegIndex, View, TileGroup, FloatFormat, CropRect, INDEX_MAGIC, INDEX_MAX_SEGS, LIB_PATH  # noqa: F401

__all__ = ["Context", "DwtxError", "compute_lengths", "geometry", "index_from_row", "tile_groups", "view_fields", "view_order", "float_format", "crop_plan",
           "view_list_fields", "view_list_check", "view_flips", "view_flip_plan",
           "Geom", "Stats", "View", "TileGroup", "FloatFormat", "CropRect"]


class DwtxError(RuntimeError):
    def __init__(self, rc, what):
        msg = _lib.load().dwtx_last_error().decode(errors="replace")
        super().__init__(f"{what} failed with {rc}: {msg}")
        self.rc = rc


def _check(rc, what):
    if rc != 0:
        raise DwtxError(rc, what)


def compute_lengths(W, H, N0=8):
    """utils.h:28 compute_lengths -> (levels, lengths, pixels, widths, heights)."""
    lib = _lib.load()
    arr = [(C.c_int * 16)() for _ in range(4)]
    levels = lib.dwtx_compute_lengths(arr[0], arr[1], arr[2], arr[3], W, H, N0)
    return (levels,) + tuple(list(a[: levels + 1]) for a in arr)


def geometry(W, H):
    g = Geom()
    _check(_lib.load().dwtx_geometry(C.byref(g), W, H), "dwtx_geometry")
    return g


def tile_groups(W, H, tile):
    """dwtx_tile_groups: the 1 to 4 same-geometry groups (TileGroup) of a W x H frame cut into `tile`-sided tiles —
    interior, right column, bottom row, corner.  Host arithmetic only."""
    out = (TileGroup * 4)()
    k = _lib.load().dwtx_tile_groups(W, H, tile, out)
    if k < 0:
        raise DwtxError(k, "dwtx_tile_groups")
    return [TileGroup.from_buffer_copy(bytes(out[i])) for i in range(k)]


def crop_plan(W, H, x0, y0, cw, ch):
    """dwtx_crop_plan: the rectangles (x0, y0, w, h) of the LL band of every level, root first and the crop itself last, that
    the cw x ch crop at (x0, y0) of a W x H picture needs.  Host arithmetic only."""
    out = (CropRect * (_lib.MAX_LEVELS + 1))()
    k = _lib.load().dwtx_crop_plan(W, H, x0, y0, cw, ch, out)
    if k < 0:
        raise DwtxError(k, "dwtx_crop_plan")
    return [(r.x0, r.y0, r.w, r.h) for r in out[:k + 1]]


ORDERS = {"rgb": 0, "bgr": 1}   # enum DWTX_ORDER_* (include/dwtx.h)


def view_order(order):
    """The `order` keyword of encode_view / decode_view -> DWTX_ORDER_*: "rgb", or "bgr" for pixels (or planes) that lie as
    B, G, R.  Anything else is a ValueError — raised here, before any device call."""
    if not isinstance(order, str) or order not in ORDERS:
        raise ValueError(f"order {order!r}: a view's channels lie as 'rgb' or as 'bgr'")
    return ORDERS[order]


FLOAT_TYPES = {"float32": 0, "float16": 1, "bfloat16": 2}   # enum DWTX_FLOAT32 / _FLOAT16 / _BFLOAT16 (include/dwtx.h)


def float_format(dtype, scale=1.0, bias=0.0):
    """The dtype, `scale` and `bias` keywords of decode_view_float and encode_view_float -> FloatFormat.  dtype:
    torch.float32 / float16 / bfloat16 (or their names); scale and bias: a number, or three — one per COLOUR, R, G, B, whatever order the channels lie in.  The
    values are rounded to float32 here, as the library holds them.  Anything else — another dtype, another length, a value
    that is not finite (before or after that rounding) — is a ValueError, raised here, before any device call."""
    import math
    import struct

    name = str(dtype).replace("torch.", "")
    if name not in FLOAT_TYPES:
        raise ValueError(f"dtype {dtype}: a float view holds float32, float16 or bfloat16 samples")
    fmt = FloatFormat(FLOAT_TYPES[name])
    for what, arg, dst in (("scale", scale, fmt.scale), ("bias", bias, fmt.bias)):
        try:
            vals = [float(v) for v in arg]
        except TypeError:
            vals = [float(arg)] * 3
        if len(vals) != 3:
            raise ValueError(f"{what}: one value or three (R, G, B), not {len(vals)}")
        for c, v in enumerate(vals):
            try:
                v32 = struct.unpack("f", struct.pack("f", v))[0]
            except OverflowError:
                v32 = math.inf
            if not math.isfinite(v32):
                raise ValueError(f"{what}[{c}] = {v!r} is not a finite float32")
            dst[c] = v32
    return fmt


def view_fields(shape, strides, stepped=False):
    """Shape and strides (in samples) of a tensor [n,H,W,C] or [bands,cols,H,W,C] -> the fields of its dwtx_view and its
    pixel step: a dict with W, H, channels, n, cols, row_pitch, image_stride, band_stride, channel_stride and pixel_step
    (0: dense).  Needs no device.  RGB pixels are interleaved (channel stride 1, column stride 3) or planar (column stride 1,
    any channel stride).  stepped=True also takes pixels that lie further apart than their own samples — RGB with channel
    stride 1 and a column stride of 3 or more (`rgba[..., :3]`), one channel with any column stride of 1 or more
    (`rgba[..., 3:]`, `uv[:, :, 0::2]`) — and reports the column stride as pixel_step, for the *_view_step calls."""
    if len(shape) not in (4, 5) or len(strides) != len(shape):
        raise ValueError("a view needs a tensor [n,H,W,C] or [bands,cols,H,W,C]")
    H, W, Cn = shape[-3:]
    sh, sw, sc = strides[-3:]
    planar = Cn == 3 and sw == 1 and sc >= 1
    step = 0
    if Cn in (1, 3) and not planar and stepped and sw >= Cn and (Cn == 1 or sc == 1):
        step = 0 if sw == Cn else sw
    elif Cn not in (1, 3) or not (planar or (sw == Cn and (Cn == 1 or sc == 1))):
        raise ValueError("a view needs 1 or 3 channels, RGB pixels either interleaved (channel stride 1, column stride 3) or planar "
                         f"(column stride 1, any channel stride), not channel stride {sc} and column stride {sw} (C = {Cn})")
    if len(shape) == 4:
        n, cols, band = shape[0], 0, 0
    else:
        n, cols, band = shape[0] * shape[1], shape[1], strides[0]
    return dict(W=W, H=H, channels=Cn, n=n, cols=cols, row_pitch=sh, image_stride=strides[-4], band_stride=band,
                channel_stride=sc if planar else 0, pixel_step=step)


def view_list_fields(windows, stepped=False):
    """A sequence of n tensors [H,W,C] — separately allocated pictures, slices of a frame, permuted [C,H,W] tensors — of
    one shape, one set of strides, one dtype and one device -> (fields, pointers): view_fields of the shape with a leading
    1 (n set to the list's length; cols, image_stride and band_stride say nothing of a list), and the tensors' data
    pointers.  A ValueError names the first tensor that differs from the first one."""
    ws = list(windows)
    if not ws:
        raise ValueError("a window list needs at least one tensor")
    t0 = ws[0]
    if len(t0.shape) != 3:
        raise ValueError(f"a window list holds tensors [H,W,C], not {tuple(t0.shape)}")
    key0 = (t0.shape, t0.stride(), t0.dtype, t0.device)
    for i, t in enumerate(ws):
        if (t.shape, t.stride(), t.dtype, t.device) == key0:   # (one comparison per window: a list may hold thousands)
            continue
        for what, a, b in (("shape", tuple(t.shape), tuple(t0.shape)), ("strides", tuple(t.stride()), tuple(t0.stride())),
                           ("dtype", t.dtype, t0.dtype), ("device", t.device, t0.device)):
            if a != b:
                raise ValueError(f"window {i} has {what} {a}, window 0 has {b}: the windows of a list share them")
    f = view_fields((1,) + tuple(t0.shape), (0,) + tuple(t0.stride()), stepped)
    f.update(n=len(ws), cols=0, image_stride=0, band_stride=0)
    return f, [t.data_ptr() for t in ws]


def view_list_check(pointers, W, H, channels=1, row_pitch=None, channel_stride=0, pixel_step=0, sample_bytes=1, maxval=None, dst=True):
    """dwtx_view_list_check: what encode_view_list (dst=False) and decode_view_list (dst=True) say to n windows of W x H at
    `pointers` (plain integers, never dereferenced; None or 0: a NULL entry) -> (rc, text): (0, "") for a list they take,
    else the error code and the text of the refusal.  Strides count samples, as in view_fields; row_pitch None: dense
    rows.  Host arithmetic only: needs no device."""
    lib = _lib.load()
    if row_pitch is None:
        row_pitch = W if channels == 3 and channel_stride else ((W - 1) * pixel_step + channels if pixel_step else W * channels)
    if maxval is None:
        maxval = 255 if sample_bytes == 1 else 65535
    v = View(None, sample_bytes, channels, maxval, 0, row_pitch, 0, 0, channel_stride)
    ptrs = list(pointers)
    arr = (C.c_void_p * max(len(ptrs), 1))(*[p or None for p in ptrs])
    rc = lib.dwtx_view_list_check(C.byref(v), pixel_step, W, H, len(ptrs), arr, 1 if dst else 0)
    return rc, (lib.dwtx_last_error().decode(errors="replace") if rc else "")


def view_delta_check(fields, base_fields, pointer, base_pointer, sample_bytes=1, base_sample_bytes=None, signed=False, minval=0, maxval=None, dst=True):
    """dwtx_view_delta_check: what encode_view (dst=False) and decode_view (dst=True) with base= say to two grid views ->
    (rc, text): (0, "") for a pair they take, else the error code and the text of the refusal.  fields, base_fields:
    view_fields dicts (strides in samples) of the view and of its base; pointer, base_pointer: their first samples' addresses
    as plain integers, never dereferenced.  Host arithmetic only: needs no device."""
    lib = _lib.load()
    if base_sample_bytes is None:
        base_sample_bytes = sample_bytes
    if maxval is None:
        maxval = 255 if sample_bytes == 1 else 32767 if signed else 65535

    def view(f, ptr, sb):
        return View(ptr or None, sb, f["channels"], maxval, f["cols"], f["row_pitch"], f["image_stride"], f["band_stride"], f["channel_stride"])

    v, vb = view(fields, pointer, sample_bytes), view(base_fields, base_pointer, base_sample_bytes)
    rc = lib.dwtx_view_delta_check(C.byref(v), fields["pixel_step"], C.byref(vb), base_fields["pixel_step"], 1 if signed else 0, int(minval),
                                   fields["W"], fields["H"], fields["n"], 1 if dst else 0)
    return rc, (lib.dwtx_last_error().decode(errors="replace") if rc else "")


def view_chain_check(fields, key_fields, pointer, key_pointer, sample_bytes=1, key_sample_bytes=None, signed=False, minval=0, maxval=None, dst=True):
    """dwtx_view_chain_check: what encode_view_chain (dst=False) and decode_view_chain (dst=True) say to a grid view and a key ->
    (rc, text): (0, "") for a pair they take, else the error code and the text of the refusal.  fields: the view_fields dict of
    the view; key_fields: that of the key, ONE window (its n, cols, image_stride and band_stride are not looked at; None: a
    NULL key); pointer, key_pointer: the first samples' addresses as plain integers, never dereferenced.  Host arithmetic only:
    needs no device."""
    lib = _lib.load()
    if key_sample_bytes is None:
        key_sample_bytes = sample_bytes
    if maxval is None:
        maxval = 255 if sample_bytes == 1 else 32767 if signed else 65535
    v = View(pointer or None, sample_bytes, fields["channels"], maxval, fields["cols"], fields["row_pitch"], fields["image_stride"],
             fields["band_stride"], fields["channel_stride"])
    if key_fields is None:
        key, kstep = None, 0
    else:
        key = C.byref(View(key_pointer or None, key_sample_bytes, key_fields["channels"], maxval, 0, key_fields["row_pitch"], 0, 0,
                           key_fields["channel_stride"]))
        kstep = key_fields["pixel_step"]
    rc = lib.dwtx_view_chain_check(C.byref(v), fields["pixel_step"], key, kstep, 1 if signed else 0, int(minval), fields["W"], fields["H"],
                                   fields["n"], 1 if dst else 0)
    return rc, (lib.dwtx_last_error().decode(errors="replace") if rc else "")


def view_clips_check(fields, pointer, period, sample_bytes=1, signed=False, minval=0, maxval=None, dst=True):
    """dwtx_view_clips_check: what encode_view_clips (dst=False) and decode_view_clips (dst=True) say to a grid view whose every
    period-th window is a key -> (rc, text): (0, "") for a view they take, else the error code and the text of the refusal, which
    starts "clips view:".  fields: the view_fields dict of the view (None: a NULL view); pointer: its first sample's address as a
    plain integer, never dereferenced.  Host arithmetic only: needs no device."""
    lib = _lib.load()
    if maxval is None:
        maxval = 255 if sample_bytes == 1 else 32767 if signed else 65535
    if fields is None:
        rc = lib.dwtx_view_clips_check(None, 0, int(period), 1 if signed else 0, int(minval), 8, 8, 1, 1 if dst else 0)
    else:
        v = View(pointer or None, sample_bytes, fields["channels"], maxval, fields["cols"], fields["row_pitch"], fields["image_stride"],
                 fields["band_stride"], fields["channel_stride"])
        rc = lib.dwtx_view_clips_check(C.byref(v), fields["pixel_step"], int(period), 1 if signed else 0, int(minval), fields["W"], fields["H"],
                                       fields["n"], 1 if dst else 0)
    return rc, (lib.dwtx_last_error().decode(errors="replace") if rc else "")


def clip_origins(origins, n, period):
    """The `origins` keyword of decode_view_clips_crop -> the list of ceil(n / period) (x0, y0) pairs, one per CLIP, or None for
    all (0, 0): one pair for every clip, or a sequence of one pair per clip.  A wrong number of pairs is a ValueError."""
    nclips = -(-int(n) // int(period))
    if origins is None:
        return None
    flat = [int(c) for c in origins] if len(origins) == 2 and not hasattr(origins[0], "__len__") else None
    pairs = [tuple(flat)] * nclips if flat is not None else [(int(x), int(y)) for x, y in origins]
    if len(pairs) != nclips:
        raise ValueError(f"origins: one (x0, y0) pair or one per clip ({nclips} clips of period {period} in {n} windows), not {len(pairs)}")
    return pairs


def view_clips_crop_check(fields, pointer, period, size, origins=None, sample_bytes=1, signed=False, minval=0, maxval=None, fmt=None):
    """dwtx_view_clips_crop_check: what decode_view_clips_crop says to a grid view of crop-sized windows (fields: its view_fields
    dict, whose W and H are the crop's; None: a NULL view), streams of geometry size=(W, H), origins (a flat or nested sequence of
    one pair per clip, passed as it is; None: NULL) and fmt (a FloatFormat, or None for integer samples) -> (rc, text): (0, "") for
    a call it takes, else the error code and the text of the refusal, which starts "clips view:".  pointer: the view's first
    sample's address as a plain integer, never dereferenced.  Host arithmetic only: needs no device."""
    lib = _lib.load()
    if maxval is None:
        maxval = 255 if sample_bytes == 1 or fmt is not None else 32767 if signed else 65535
    W, H = (int(v) for v in size)
    org = None
    if origins is not None:
        flat = [int(c) for p in origins for c in (p if hasattr(p, "__len__") else (p,))]
        org = (C.c_int * max(len(flat), 1))(*flat)
    pf = C.byref(fmt) if fmt is not None else None
    if fields is None:
        rc = lib.dwtx_view_clips_crop_check(None, 0, int(period), 1 if signed else 0, int(minval), pf, W, H, 1, W, H, org)
    else:
        v = View(pointer or None, sample_bytes, fields["channels"], maxval, fields["cols"], fields["row_pitch"], fields["image_stride"],
                 fields["band_stride"], fields["channel_stride"])
        rc = lib.dwtx_view_clips_crop_check(C.byref(v), fields["pixel_step"], int(period), 1 if signed else 0, int(minval), pf, W, H,
                                            fields["n"], fields["W"], fields["H"], org)
    return rc, (lib.dwtx_last_error().decode(errors="replace") if rc else "")


FLIPS = {"": 0, "x": 1, "y": 2, "xy": 3, "yx": 3}   # enum DWTX_FLIP_X = 1, DWTX_FLIP_Y = 2 (include/dwtx.h): a mask


def _flip_flag(f):
    if isinstance(f, str) and f in FLIPS:
        return FLIPS[f]
    if f is None:
        return 0
    if isinstance(f, bool) or not hasattr(f, "__index__") or not 0 <= int(f) <= 3:
        raise ValueError(f"flip {f!r}: None, 0, 'x', 'y', 'xy' or a mask 1..3 (x = 1, y = 2)")
    return int(f)


def view_flips(flip, n):
    """The `flip` keyword of the view calls -> None when no window is flipped (None, 0, or a sequence of zeros: the call
    made is the one made without the keyword), else (flip, flips) for the *_view_flip calls: one mask for all windows and
    None, or 0 and a ctypes array of n masks.  Takes None, 0, "x", "y", "xy", 1..3 (x = 1, y = 2), or a sequence of n of
    those (a tensor or an array of integers too).  Anything else is a ValueError — raised here, before any device call."""
    if flip is None or isinstance(flip, (str, int)) or (hasattr(flip, "__index__") and not hasattr(flip, "__len__")):
        f = _flip_flag(flip)
        return (f, None) if f else None
    if hasattr(flip, "tolist"):
        flip = flip.tolist()
    try:
        flags = [_flip_flag(f) for f in flip]
    except TypeError:
        raise ValueError(f"flip {flip!r}: one value or a sequence of {n}") from None
    if len(flags) != n:
        raise ValueError(f"flip: one value or {n}, one per window, not {len(flags)}")
    if not any(flags):
        return None
    return 0, (C.c_ubyte * n)(*flags)


def view_flip_plan(W, H, n, flip, pointers=None, channels=1, row_pitch=None, image_stride=None, cols=0, band_stride=0, channel_stride=0,
                   pixel_step=0, sample_bytes=1, maxval=None, dst=True, flips=None):
    """dwtx_view_flip_plan: what a flipped encode (dst=False) or decode (dst=True) says to n windows of W x H — at `pointers`
    (plain integers, never dereferenced), or, pointers None, on the grid that cols, image_stride and band_stride describe —
    and the table it walks them with -> (rc, text, origin, pitch, step): rc 0 and "" for a call it takes, else the error
    code and the text of the refusal (and three empty lists).  origin[i]: where pixel (0, 0) of window i's picture lies, in
    samples from the grid's first sample or from the lowest pointer; pitch[i], step[i]: the signed row pitch and pixel step
    the picture is walked with from there.  flip: one mask 0..3 for all windows; flips: a sequence of n masks instead — both
    go to the library as they are, a refusal is the library's.  Strides count samples; row_pitch None: dense rows,
    image_stride None: dense windows.  Host arithmetic only: needs no device."""
    lib = _lib.load()
    if row_pitch is None:
        row_pitch = W if channels == 3 and channel_stride else ((W - 1) * pixel_step + channels if pixel_step else W * channels)
    if image_stride is None:
        image_stride = row_pitch * H
    if maxval is None:
        maxval = 255 if sample_bytes == 1 else 65535
    arr = None
    if pointers is not None:
        ptrs = list(pointers)
        arr = (C.c_void_p * max(len(ptrs), 1))(*[p or None for p in ptrs])
    v = View(None if arr is not None else 4096, sample_bytes, channels, maxval, cols, row_pitch, image_stride, band_stride, channel_stride)
    fl = None if flips is None else (C.c_ubyte * max(len(flips), 1))(*[int(f) for f in flips])
    out = [(C.c_longlong * max(n, 1))() for _ in range(3)]
    rc = lib.dwtx_view_flip_plan(C.byref(v), pixel_step, W, H, n, arr, int(flip), fl, 1 if dst else 0, *out)
    if rc:
        return rc, lib.dwtx_last_error().decode(errors="replace"), [], [], []
    return (0, "") + tuple(list(a[:n]) for a in out)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def index_from_row(row):
    """One row of the device tensor of Context.set_encode_index(device=True) (uint8, sizeof(Index) bytes; a torch tensor
    or anything bytes() takes) -> Index."""
    if hasattr(row, "cpu"):
        row = row.cpu().numpy().tobytes()
    return Index.from_buffer_copy(bytes(row))


class Context:
    """One HIP device + stream + scratch arena (dwtx_ctx)."""

    def __init__(self, device=0, stream=None):
        import torch

        self.torch = torch
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("dwt_amd needs a HIP device; there is no CPU path")
        self.device = torch.device("cuda", device)
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        h = C.c_void_p()
        _check(self.lib.dwtx_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)), "dwtx_ctx_create_on_stream")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.dwtx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name, value=1):
        """Diagnostic switch of the context (enum dwtx_option in include/dwtx.h; tests and tools only)."""
        _check(self.lib.dwtx_ctx_set_option(self.h, _lib.OPTIONS[name], int(value)), "dwtx_ctx_set_option")

    def get_option(self, name):
        return self.lib.dwtx_ctx_get_option(self.h, _lib.OPTIONS[name])

    def set_index(self, offered=None, wanted=0):
        """Sidecar indices for the decode calls that follow (dwtx_ctx_set_index): `offered` is an array of Index
        made by new_indices()/an earlier decode (entry i goes with image i of a call), `wanted` the number of
        entries to collect.  Returns the array that will receive them (or None).  set_index() ends it."""
        out = (Index * wanted)() if wanted else None
        self._index = (offered, out)   # the library keeps the pointers
        _check(self.lib.dwtx_ctx_set_index(self.h, C.cast(offered, C.c_void_p) if offered is not None else None,
                                           C.cast(out, C.c_void_p) if out is not None else None), "dwtx_ctx_set_index")
        return out

    def set_encode_index(self, wanted=0, device=False):
        """Sidecar indices from the encode calls that follow (dwtx_ctx_set_encode_index): entry i receives the index of
        image i of a call.  device=False: a ctypes array of `wanted` Index entries, for encode() (host buffers);
        device=True: a uint8 device tensor [wanted, sizeof(Index)], for encode_planes() / encode_device(), written on the
        context's stream like the info records (index_from_row() reads a downloaded row).  Entries are not cleared: an
        encode writes an entry's header and seg[:nsegs].  set_encode_index() ends it."""
        if not wanted:
            out, ptr = None, None
        elif device:
            out = self.torch.empty((wanted, C.sizeof(Index)), dtype=self.torch.uint8, device=self.device)
            ptr = _ptr(out)
        else:
            out = (Index * wanted)()
            ptr = C.cast(out, C.c_void_p)
        self._encode_index = out   # the library keeps the pointer
        _check(self.lib.dwtx_ctx_set_encode_index(self.h, ptr), "dwtx_ctx_set_encode_index")
        return out

    def sync(self):
        _check(self.lib.dwtx_sync(self.h), "dwtx_sync")

    def synth_pixels(self, n, H, W, C_, seed0=0, kind=0):
        """Synthetic uint8 frames [n,H,W,C] rendered on the device (SURVEY.md §8d generator)."""
        out = self.torch.empty((n, H, W, C_), dtype=self.torch.uint8, device=self.device)
        _check(self.lib.dwtx_synth_pixels(self.h, _ptr(out), W, H, C_, n, seed0, kind), "dwtx_synth_pixels")
        return out

    # -- stage kernels -------------------------------------------------------

    def _planes_from_pixels(self, sym, pix):
        n, H, W, Cn = pix.shape
        out = self.torch.empty((n * Cn, H, W), dtype=self.torch.int32, device=self.device)
        _check(getattr(self.lib, sym)(self.h, _ptr(out), _ptr(pix), W, H, Cn, n), sym)
        return out

    def _pixels_from_planes(self, sym, dtype, planes, C_, *maxval):
        nC, H, W = planes.shape
        n = nC // C_
        assert planes.dtype == self.torch.int32 and planes.is_contiguous()
        out = self.torch.empty((n, H, W, C_), dtype=dtype, device=self.device)
        _check(getattr(self.lib, sym)(self.h, _ptr(out), _ptr(planes), W, H, C_, n, *maxval), sym)
        return out

    def planes_from_pixels(self, pix):
        """uint8 [n,H,W,C] interleaved -> int32 [n*C,H,W] planar (YCoCg-R if C==3)."""
        assert pix.dtype == self.torch.uint8 and pix.is_contiguous() and pix.device == self.device
        return self._planes_from_pixels("dwtx_planes_from_pixels", pix)

    def pixels_from_planes(self, planes, C_):
        return self._pixels_from_planes("dwtx_pixels_from_planes", self.torch.uint8, planes, C_)

    def transformation_fwd(self, planes, out=None):
        """encode.c:16 transformation: int32 [P,H,W] -> Mallat pyramid [P,H,W]."""
        torch = self.torch
        P, H, W = planes.shape
        assert planes.dtype == torch.int32 and planes.is_contiguous()
        if out is None:
            out = torch.empty_like(planes)
        _check(self.lib.dwtx_transformation_fwd(self.h, _ptr(out), _ptr(planes), W, H, P), "dwtx_transformation_fwd")
        return out

    def transformation_inv(self, pyr, out=None):
        """decode.c:16 transformation (inverse)."""
        torch = self.torch
        P, H, W = pyr.shape
        assert pyr.dtype == torch.int32 and pyr.is_contiguous()
        if out is None:
            out = torch.empty_like(pyr)
        _check(self.lib.dwtx_transformation_inv(self.h, _ptr(out), _ptr(pyr), W, H, P), "dwtx_transformation_inv")
        return out

    def transformation_fwd_pixels(self, pix, rings16=True, out=None):
        """encode.c:155-159 in one pass as dwtx_encode_device runs it: uint8 [n,H,W,C] -> (int32 pyramid [n*C,H,W],
        int16 planes [n*C,H,W] or None, mask of the ring levels that live in the int16 planes)."""
        torch = self.torch
        n, H, W, Cn = pix.shape
        assert pix.dtype == torch.uint8 and pix.is_contiguous()
        pyr, r16 = out if out is not None else (None, None)
        if pyr is None:
            pyr = torch.zeros((n * Cn, H, W), dtype=torch.int32, device=pix.device)
        if rings16 and r16 is None:
            r16 = torch.zeros((n * Cn, H, W), dtype=torch.int16, device=pix.device)
        mask = C.c_uint(0)
        _check(self.lib.dwtx_transformation_fwd_pixels(self.h, _ptr(pyr), _ptr(r16) if rings16 else None, C.byref(mask), _ptr(pix),
                                                       W, H, Cn, n), "dwtx_transformation_fwd_pixels")
        return pyr, (r16 if rings16 else None), mask.value

    def transformation_inv_pixels(self, pyr, r16, mask, Cn, out=None):
        """decode.c:258-264 as dwtx_decode_device runs it: (pyramid, int16 ring planes, mask) -> uint8 [n,H,W,C]."""
        torch = self.torch
        P, H, W = pyr.shape
        n = P // Cn
        if out is None:
            out = torch.empty((n, H, W, Cn), dtype=torch.uint8, device=pyr.device)
        _check(self.lib.dwtx_transformation_inv_pixels(self.h, _ptr(out), _ptr(pyr), _ptr(r16) if mask else None, mask, W, H, Cn, n),
               "dwtx_transformation_inv_pixels")
        return out

    def linearization(self, pyr):
        """encode.c:32 linearization: pyramid [P,H,W] -> Hilbert-linearised [P,H*W]."""
        torch = self.torch
        P, H, W = pyr.shape
        assert pyr.dtype == torch.int32 and pyr.is_contiguous()
        out = torch.empty((P, H * W), dtype=torch.int32, device=self.device)
        _check(self.lib.dwtx_linearization(self.h, _ptr(out), _ptr(pyr), W, H, P), "dwtx_linearization")
        return out

    def reconstruction(self, lin, W, H, C_, levels_out=None, missing=None):
        """decode.c:32 reconstruction: [n*C, W*H] -> pyramid [n*C, h', w'] of the first levels_out levels."""
        torch = self.torch
        P = lin.shape[0]
        n = P // C_
        g = geometry(W, H)
        if levels_out is None:
            levels_out = g.levels
        ow, oh = g.widths[levels_out], g.heights[levels_out]
        out = torch.empty((P, oh, ow), dtype=torch.int32, device=self.device)
        mp = C.c_void_p(0)
        if missing is not None:
            assert missing.dtype == torch.int32 and missing.numel() == n * 48 and missing.is_contiguous()
            mp = _ptr(missing)
        _check(self.lib.dwtx_reconstruction(self.h, _ptr(out), _ptr(lin), mp, levels_out, W, H, C_, n),
               "dwtx_reconstruction")
        return out

    def encode_planes(self, lin, W, H, C_, capacity=0, out_stride=None):
        """encode.c:166-221 on linearised planes [n*C, W*H] -> (list of bytes, list of StreamInfo)."""
        import numpy as np

        torch = self.torch
        n = lin.shape[0] // C_
        assert lin.dtype == torch.int32 and lin.is_contiguous()
        if out_stride is None:
            out_stride = capacity if capacity > 0 else 2 * W * H * C_ + 4096
            out_stride = (out_stride + 8 + 3) // 4 * 4
        out = torch.empty((n, out_stride), dtype=torch.uint8, device=self.device)
        info = torch.empty((n, C.sizeof(StreamInfo)), dtype=torch.uint8, device=self.device)
        _check(self.lib.dwtx_encode_planes(self.h, _ptr(lin), W, H, C_, n, capacity, _ptr(out), out_stride, _ptr(info)),
               "dwtx_encode_planes")
        raw = info.cpu().numpy()
        infos = [StreamInfo.from_buffer_copy(raw[i].tobytes()) for i in range(n)]
        host = out.cpu().numpy()
        streams = []
        for i in range(n):
            if infos[i].error:
                raise DwtxError(-3, "dwtx_encode_planes (more than 16 bit planes)")
            if infos[i].nbytes > out_stride:
                raise DwtxError(-2, "dwtx_encode_planes (out_stride too small)")
            streams.append(host[i, : infos[i].nbytes].tobytes())
        return streams, infos

    def decode_planes(self, streams, W, H, C_, levels_max=-1):
        """decode.c:174-250 on a list of .dwt byte strings of one geometry ->
        (lin int32 [n*C, W*H] two's complement, list of DecodeInfo)."""
        import numpy as np

        torch = self.torch
        n = len(streams)
        stride = (max(len(s) for s in streams) + 64 + 7) // 8 * 8
        host = np.zeros((n, stride), dtype=np.uint8)
        for i, s in enumerate(streams):
            host[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
        dev = torch.from_numpy(host).to(self.device)
        lens = torch.tensor([len(s) for s in streams], dtype=torch.int64, device=self.device)
        lin = torch.empty((n * C_, W * H), dtype=torch.int32, device=self.device)
        infos = (DecodeInfo * n)()
        _check(self.lib.dwtx_decode_planes(self.h, _ptr(lin), _ptr(dev), stride, _ptr(lens), W, H, C_, n, levels_max,
                                           C.cast(infos, C.c_void_p)), "dwtx_decode_planes")
        self._keep = (dev, lens)   # kernels after the internal sync still read the streams
        return lin, list(infos)

    # -- whole images (host numpy in/out; what the CLIs do) ---------------------

    def _encode(self, sym, dtype, bound, pix, capacity):
        import numpy as np

        single = pix.ndim == 3
        pix = np.ascontiguousarray(pix[None] if single else pix, dtype=dtype)
        n, H, W, Cn = pix.shape
        stride = bound(W, H, Cn) if capacity <= 0 else (capacity + 15) // 8 * 8
        out = np.empty((n, stride), dtype=np.uint8)
        lens = (C.c_size_t * n)()
        stats = (Stats * n)()
        _check(getattr(self.lib, sym)(self.h, pix.ctypes.data, W, H, Cn, n, capacity, out.ctypes.data, stride,
                                      C.cast(lens, C.c_void_p), C.cast(stats, C.c_void_p)), sym)
        streams = [out[i, : lens[i]].tobytes() for i in range(n)]
        return (streams[0], stats[0]) if single else (streams, list(stats))

    def _decode(self, sym, dtype, streams, pixels_max, maxval=None, minval=None):
        """maxval None: bytes; else deep pixels, whose symbol takes maxval (signed ones: minval before it) and (unused here)
        an array of DecodeInfo."""
        import numpy as np

        single = isinstance(streams, (bytes, bytearray))
        lst = [streams] if single else list(streams)
        n = len(lst)
        if len(lst[0]) < 6:
            raise DwtxError(-3, sym + " (short header)")
        W = (lst[0][2] | (lst[0][3] << 8)) + 1
        H = (lst[0][4] | (lst[0][5] << 8)) + 1
        Cn = 3 if lst[0][1:2] == b"6" else 1
        stride = (max(len(s) for s in lst) + 64 + 7) // 8 * 8
        host = np.zeros((n, stride), dtype=np.uint8)
        for i, s in enumerate(lst):
            host[i, : len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        lens = (C.c_size_t * n)(*[len(s) for s in lst])
        pstride = W * H * Cn
        pix = np.empty((n, pstride), dtype=dtype)
        ow, oh, oc = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
        sizes = (ow, oh, oc) if maxval is None else (maxval, ow, oh, oc, None) if minval is None else (minval, maxval, ow, oh, oc, None)
        rc = getattr(self.lib, sym)(self.h, host.ctypes.data, stride, C.cast(lens, C.c_void_p), n, pixels_max,
                                    pix.ctypes.data, pstride, *sizes)
        if rc == -1 and n == 1:   # one unreadable stream is an error code (decode.c exits 1), in a batch it is a missing picture
            return None if single else [None]
        _check(rc, sym)
        outs = [pix[i, : ow[i] * oh[i] * oc[i]].reshape(oh[i], ow[i], oc[i]).copy() if ow[i] else None for i in range(n)]
        return outs[0] if single else outs

    def encode(self, pix, capacity=0):
        """uint8 numpy [n,H,W,C] (or [H,W,C]) -> list of .dwt byte strings, list of Stats."""
        import numpy as np

        return self._encode("dwtx_encode_images", np.uint8, self.lib.dwtx_encode_bound, pix, capacity)

    def decode(self, streams, pixels_max=-1):
        """.dwt byte string (or list of same-geometry ones) -> uint8 numpy [h,w,C] (or list); None if unreadable."""
        import numpy as np

        return self._decode("dwtx_decode_images", np.uint8, streams, pixels_max)

    # -- whole images, device resident (what bench.py times) --------------------

    def _encode_device(self, sym, bound, pix, capacity, out, info):
        torch = self.torch
        n, H, W, Cn = pix.shape
        stride = bound(W, H, Cn) if capacity <= 0 else (capacity + 15) // 8 * 8
        if out is None:
            out = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
        if info is None:
            info = torch.empty((n, C.sizeof(StreamInfo)), dtype=torch.uint8, device=self.device)
        _check(getattr(self.lib, sym)(self.h, _ptr(pix), W, H, Cn, n, capacity, _ptr(out), out.shape[1], _ptr(info)), sym)
        return out, info

    def encode_device(self, pix, capacity=0, out=None, info=None):
        """uint8 device tensor [n,H,W,C] -> (streams uint8 [n,stride], info uint8 [n,sizeof(StreamInfo)]) on device; async."""
        assert pix.dtype == self.torch.uint8 and pix.is_contiguous()
        return self._encode_device("dwtx_encode_device", self.lib.dwtx_encode_bound, pix, capacity, out, info)

    def stream_lengths(self, info):
        """int64 device tensor of stream byte lengths from the info records of encode_device."""
        off = StreamInfo.nbytes.offset
        return info[:, off:off + 8].contiguous().view(self.torch.int64).view(-1)

    def pack_streams(self, streams, lens, out, offsets=None):
        """dwtx_pack_streams: the n streams of a batch (uint8 [n, stride], int64 lens on the device) moved together into the
        flat uint8 tensor `out`, stream i at sum(round8(lens[:i])); offsets: optional int64 [n + 1] device tensor."""
        torch = self.torch
        n, stride = streams.shape
        assert streams.dtype == torch.uint8 and streams.is_contiguous() and out.dtype == torch.uint8 and out.is_contiguous()
        assert lens.dtype == torch.int64 and lens.numel() == n and lens.is_contiguous()
        assert offsets is None or (offsets.dtype == torch.int64 and offsets.numel() == n + 1)
        _check(self.lib.dwtx_pack_streams(self.h, _ptr(out), out.numel(), _ptr(offsets) if offsets is not None else None,
                                          _ptr(streams), stride, _ptr(lens), n), "dwtx_pack_streams")
        return out

    def _decode_device(self, sym, dtype, streams, lens, W, H, C_, levels_max, out, maxval=None):
        """maxval None: bytes, slots of W*H*C samples; else deep pixels, slots of out.shape[1] samples."""
        torch = self.torch
        n, stride = streams.shape
        assert streams.dtype == torch.uint8 and streams.is_contiguous() and stride % 8 == 0
        assert lens.dtype == torch.int64 and lens.numel() == n
        if out is None:
            out = torch.empty((n, W * H * C_), dtype=dtype, device=self.device)
        if maxval is None:
            slot = (W * H * C_,)
        else:
            assert self._is16(out) and out.shape[0] == n
            slot = (out.shape[1], maxval)
        infos = (DecodeInfo * n)()
        _check(getattr(self.lib, sym)(self.h, _ptr(streams), stride, _ptr(lens), W, H, C_, n, levels_max,
                                      _ptr(out), *slot, C.cast(infos, C.c_void_p)), sym)
        return out, list(infos)

    def decode_device(self, streams, lens, W, H, C_, levels_max=-1, out=None):
        """device streams [n,stride] + int64 lens -> (uint8 [n, W*H*C] pixels, list of DecodeInfo); syncs once."""
        return self._decode_device("dwtx_decode_device", self.torch.uint8, streams, lens, W, H, C_, levels_max, out)

    # -- deep pixels: uint16 samples, maxval up to 65535 (the *16 calls of include/dwtx.h) -----------------------
    # torch's uint16 has few operators on the device, so deep device tensors may be torch.uint16 or torch.int16
    # (the same two bytes); results come back as torch.uint16.

    def _is16(self, t):
        return t.dtype in (self.torch.uint16, self.torch.int16) and t.is_contiguous() and t.device == self.device

    def planes_from_pixels16(self, pix):
        """16-bit [n,H,W,C] interleaved device tensor -> int32 [n*C,H,W] planar (YCoCg-R if C==3)."""
        assert self._is16(pix)
        return self._planes_from_pixels("dwtx_planes_from_pixels16", pix)

    def pixels16_from_planes(self, planes, C_, maxval):
        """int32 [n*C,H,W] -> uint16 [n,H,W,C] with the reference's clamps at maxval."""
        return self._pixels_from_planes("dwtx_pixels16_from_planes", self.torch.uint16, planes, C_, maxval)

    def transformation_fwd_pixels16(self, pix, out=None):
        """encode.c:155-159 for deep pixels: 16-bit [n,H,W,C] -> int32 pyramid [n*C,H,W]."""
        torch = self.torch
        n, H, W, Cn = pix.shape
        assert self._is16(pix)
        if out is None:
            out = torch.empty((n * Cn, H, W), dtype=torch.int32, device=self.device)
        _check(self.lib.dwtx_transformation_fwd_pixels16(self.h, _ptr(out), _ptr(pix), W, H, Cn, n), "dwtx_transformation_fwd_pixels16")
        return out

    def transformation_inv_pixels16(self, pyr, Cn, maxval, out=None):
        """decode.c:258-264 for deep pixels: int32 pyramid [n*C,H,W] -> uint16 [n,H,W,C], clamps at maxval."""
        torch = self.torch
        P, H, W = pyr.shape
        n = P // Cn
        assert pyr.dtype == torch.int32 and pyr.is_contiguous()
        if out is None:
            out = torch.empty((n, H, W, Cn), dtype=torch.uint16, device=self.device)
        _check(self.lib.dwtx_transformation_inv_pixels16(self.h, _ptr(out), _ptr(pyr), W, H, Cn, n, maxval),
               "dwtx_transformation_inv_pixels16")
        return out

    def encode16(self, pix, capacity=0):
        """uint16 numpy [n,H,W,C] (or [H,W,C]) -> list of .dwt byte strings, list of Stats.  A picture that needs more
        than 16 bit planes raises DwtxError (rc -3)."""
        import numpy as np

        return self._encode("dwtx_encode_images16", np.uint16, self.lib.dwtx_encode_bound16, pix, capacity)

    def decode16(self, streams, maxval, pixels_max=-1):
        """.dwt byte string (or list of same-geometry ones) -> uint16 numpy [h,w,C] (or list); None if unreadable.
        maxval (1..65535) is what the pictures were encoded from: a .dwt does not record it."""
        import numpy as np

        return self._decode("dwtx_decode_images16", np.uint16, streams, pixels_max, maxval)

    def encode16s(self, pix, capacity=0):
        """int16 numpy [n,H,W,C] (or [H,W,C]) -> list of .dwt byte strings, list of Stats: dwtx_encode_images_s16, the signed
        integers coded as they are.  A picture that needs more than 16 bit planes raises DwtxError (rc -3)."""
        import numpy as np

        if np.asarray(pix).dtype != np.int16:
            raise ValueError(f"encode16s reads int16 pictures, not {np.asarray(pix).dtype}")
        return self._encode("dwtx_encode_images_s16", np.int16, self.lib.dwtx_encode_bound16, pix, capacity)

    def decode16s(self, streams, minval=-32768, maxval=32767, pixels_max=-1):
        """.dwt byte string (or list of same-geometry ones) -> int16 numpy [h,w,C] (or list); None if unreadable:
        dwtx_decode_images_s16.  [minval, maxval] is the range the pictures were encoded from (a .dwt does not record it):
        what the clamps of a stream that was cut short act at."""
        import numpy as np

        return self._decode("dwtx_decode_images_s16", np.int16, streams, pixels_max, int(maxval), int(minval))

    def encode_device16(self, pix, capacity=0, out=None, info=None):
        """16-bit device tensor [n,H,W,C] -> (streams uint8 [n,stride], info uint8 [n,sizeof(StreamInfo)]) on device; async."""
        assert self._is16(pix)
        return self._encode_device("dwtx_encode_device16", self.lib.dwtx_encode_bound16, pix, capacity, out, info)

    def decode_device16(self, streams, lens, W, H, C_, maxval, levels_max=-1, out=None):
        """device streams [n,stride] + int64 lens -> (uint16 [n, W*H*C] pixels, list of DecodeInfo); syncs once.
        `out`: a 16-bit device tensor [n, pix_stride] with pix_stride (in samples) >= the pictures' size."""
        return self._decode_device("dwtx_decode_device16", self.torch.uint16, streams, lens, W, H, C_, levels_max, out, maxval)

    # -- strided views: windows and tile grids of a larger frame (dwtx_encode_view / dwtx_decode_view) -----------

    def _signed_range(self, signed, minval, maxval, floats=False):
        """The `signed`, `minval` and `maxval` keywords of the view calls -> (minval or None, maxval or None): minval None means
        the unsigned call.  signed=True: int16 samples, range [-32768, 32767] unless the keywords say otherwise; float tensors
        take minval alone (0 or None: the unsigned call)."""
        if signed:
            if floats:
                raise ValueError("signed=True takes int16 tensors; float tensors take minval=")
            return (-32768 if minval is None else int(minval)), (32767 if maxval is None else int(maxval))
        if minval is not None and int(minval) != 0:
            if not floats:
                raise ValueError("minval belongs to signed=True (int16 tensors) and to float tensors")
            return int(minval), maxval
        return None, maxval

    def _view(self, t, maxval, stepped=False, floats=False, signed=False):
        """View of a strided device tensor [n,H,W,C] or [bands,cols,H,W,C] (uint8, or uint16 / int16 for deep pixels):
        the windows stay where they are.  RGB pixels are interleaved (channel stride 1, column stride 3) or planar (column
        stride 1, any channel stride): `nchw.permute(0, 2, 3, 1)` and `chw.permute(1, 2, 0)` are views as they are.
        stepped: pixels further apart than their samples too (view_fields); the last value returned is their pixel step."""
        torch = self.torch
        if floats:   # (decode_view_float, encode_view_float: the same views of float32 / float16 / bfloat16 samples)
            if t.dtype not in (torch.float32, torch.float16, torch.bfloat16) or t.device != self.device or t.dim() not in (4, 5):
                raise ValueError("a float view needs a float32 / float16 / bfloat16 tensor [n,H,W,C] or [bands,cols,H,W,C] on the context's device")
        elif signed and t.dtype != torch.int16:
            raise ValueError(f"signed=True takes int16 tensors only, not {t.dtype}")
        elif t.dtype not in (torch.uint8, torch.uint16, torch.int16) or t.device != self.device or t.dim() not in (4, 5):
            raise ValueError("a view needs a uint8 / uint16 / int16 tensor [n,H,W,C] or [bands,cols,H,W,C] on the context's device")
        f = view_fields(tuple(t.shape), tuple(t.stride()), stepped)
        deep = t.dtype != torch.uint8
        if maxval is None:
            maxval = 65535 if deep else 255
        v = View(t.data_ptr(), t.element_size(), f["channels"], maxval, f["cols"], f["row_pitch"], f["image_stride"], f["band_stride"],
                 f["channel_stride"])
        return v, f["W"], f["H"], f["channels"], f["n"], f["pixel_step"]

    def _delta_views(self, t, base, maxval, stepped, signed, flip, levels_max=-1):
        """The `base=` keyword of encode_view / decode_view -> the two views of a delta call, or a ValueError before any device
        call: flips, float tensors, levels_max, and a base of another dtype or shape than `t` are not the delta calls'."""
        torch = self.torch
        if flip is not None:
            raise ValueError("base= does not combine with flip (the delta calls take no flips)")
        if levels_max != -1:
            raise ValueError("base= does not combine with levels_max (a coarse residual has no base of its size)")
        for what, x in (("the tensor", t), ("base", base)):
            if not hasattr(x, "dtype") or x.dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
                raise ValueError(f"base= takes integer tensors: {what} holds {getattr(x, 'dtype', type(x))}")
        if base.dtype != t.dtype:
            raise ValueError(f"base= needs the tensor's dtype {t.dtype}, not {base.dtype}")
        if tuple(base.shape[-3:]) != tuple(t.shape[-3:]) or base.numel() != t.numel():   # (a grid of tiles against a stack of as many: fine)
            raise ValueError(f"base= needs the tensor's windows, {t.numel() // max(1, t[..., 0, 0, 0].numel())} of {tuple(t.shape[-3:])}, not shape {tuple(base.shape)}")
        v, W, H, Cn, n, step = self._view(t, maxval, stepped, signed=signed)
        vb, _, _, _, _, bstep = self._view(base, None, stepped, signed=signed)
        return v, vb, W, H, Cn, n, step, bstep

    def _encode_views(self, v, step, order, fmt, windows, flips, lo, W, H, n, capacity, out, info, pair=None, clips=None):
        """Every view encode: allocates `out` and `info` where the caller brought none — slots of dwtx_encode_bound, or of
        dwtx_encode_bound16 for deep, signed and delta pictures — and makes the call through the narrowest entry point that has
        the arguments given.  step: None without the `stepped` keyword; fmt, windows (a ctypes array), flips (view_flips) and lo
        (the signed calls' minval): None for a call without them; pair: (symbol, other view, its step, sgn) of a delta or chain;
        clips: (period, sgn) of a clips call, which has no other view."""
        torch = self.torch
        deep = pair is not None or clips is not None or ((v.maxval > 255 or lo is not None) if fmt is not None else v.sample_bytes == 2)
        bound = self.lib.dwtx_encode_bound16 if deep else self.lib.dwtx_encode_bound
        stride = bound(W, H, v.channels) if capacity <= 0 else (capacity + 15) // 8 * 8
        if out is None:
            out = torch.empty((n, stride), dtype=torch.uint8, device=self.device)
        if info is None:
            info = torch.empty((n, C.sizeof(StreamInfo)), dtype=torch.uint8, device=self.device)
        view = (self.h, C.byref(v), step or 0, order)
        pf = C.byref(fmt) if fmt is not None else None
        if clips is not None:
            sym, args = "dwtx_encode_view_clips", view[:3] + (clips[0], order, clips[1])
        elif pair is not None:
            sym, args = pair[0], view[:3] + (C.byref(pair[1]), pair[2], order, pair[3])
        elif lo is not None:
            fl = flips or (0, None)
            sym, args = "dwtx_encode_view_signed", view + (pf, windows, fl[0], fl[1], lo)
        elif flips:
            sym, args = "dwtx_encode_view_flip", view + (pf, windows, flips[0], flips[1])
        elif windows is not None:
            sym, args = "dwtx_encode_view_list", view + (pf, windows)
        elif fmt is not None:
            sym, args = "dwtx_encode_view_float", view + (pf,)
        elif order:
            sym, args = "dwtx_encode_view_order", view
        elif step is not None:
            sym, args = "dwtx_encode_view_step", view[:3]
        else:
            sym, args = "dwtx_encode_view", view[:2]
        _check(getattr(self.lib, sym)(*args, W, H, n, capacity, _ptr(out), out.shape[1], _ptr(info)), sym)
        return out, info

    def _decode_views(self, streams, lens, v, step, order, fmt, crop, windows, flips, lo, W, H, n, levels_max, pair=None, clips=None):
        """Every view decode, through the narrowest entry point that has the arguments given -> the list of DecodeInfo.  crop: None,
        or (cw, ch, origins as a ctypes array or None); pair: (symbol, other view, its step, sgn, minval); clips: (period, sgn,
        minval); the rest as for
        _encode_views."""
        torch = self.torch
        assert streams.dtype == torch.uint8 and streams.is_contiguous() and streams.shape[0] == n and streams.shape[1] % 8 == 0
        assert lens.dtype == torch.int64 and lens.numel() == n and lens.is_contiguous()
        infos = (DecodeInfo * n)()
        head = (self.h, _ptr(streams), streams.shape[1], _ptr(lens), W, H, n)
        view = (levels_max, C.byref(v), step or 0, order)
        pf = C.byref(fmt) if fmt is not None else None
        window = (pf,) + (crop or (W, H, None))
        if clips is not None and crop is not None:   # (its origins: one pair per clip)
            sym, args = "dwtx_decode_view_clips_crop", view[1:3] + (clips[0], order, clips[1], clips[2]) + window
        elif clips is not None:
            sym, args = "dwtx_decode_view_clips", view[1:3] + (clips[0], order, clips[1], clips[2])
        elif pair is not None:
            sym, args = pair[0], view[1:3] + (C.byref(pair[1]), pair[2], order, pair[3], pair[4])
        elif lo is not None:
            fl = flips or (0, None)
            sym, args = "dwtx_decode_view_signed", view + window + (windows, fl[0], fl[1], lo)
        elif flips:
            sym, args = "dwtx_decode_view_flip", view + window + (windows, flips[0], flips[1])
        elif windows is not None:
            sym, args = "dwtx_decode_view_list", view + window + (windows,)
        elif crop is not None:
            sym, args = "dwtx_decode_view_crop", view + window
        elif fmt is not None:
            sym, args = "dwtx_decode_view_float", view + (pf,)
        elif order:
            sym, args = "dwtx_decode_view_order", view
        elif step is not None:
            sym, args = "dwtx_decode_view_step", view[:3]
        else:
            sym, args = "dwtx_decode_view", view[:2]
        _check(getattr(self.lib, sym)(*head, *args, C.cast(infos, C.c_void_p)), sym)
        return list(infos)

    @staticmethod
    def _origins(origins, n):
        """The `origins` keyword of the crop calls -> a ctypes array of n (x0, y0) pairs, or None for (0, 0)"""
        if origins is None:
            return None
        flat = [int(c) for c in origins] if len(origins) == 2 and not hasattr(origins[0], "__len__") else None
        pairs = [tuple(flat)] * n if flat is not None else [(int(x), int(y)) for x, y in origins]
        if len(pairs) != n:
            raise ValueError(f"origins: one (x0, y0) pair or {n}, not {len(pairs)}")
        return (C.c_int * (2 * n))(*[c for p in pairs for c in p])

    def encode_view(self, t, capacity=0, out=None, info=None, stepped=False, order="rgb", flip=None, signed=False, base=None):
        """dwtx_encode_view: the windows of a strided device tensor [n,H,W,C] or [bands,cols,H,W,C] (a slice, a crop, a
        grid of tiles, a channel-first batch permuted to channel-last: see _view) -> (streams uint8 [n,stride], info uint8
        [n,sizeof(StreamInfo)]) on device, as encode_device / encode_device16 give for the contiguous copy; async.
        stepped=True: dwtx_encode_view_step — `rgba[..., :3]`, `rgba[..., 3:]` and `uv[:, :, 0::2]` are views as they lie.
        order="bgr": dwtx_encode_view_order — the channels lie as B, G, R (`bgra[..., :3]` with stepped=True, an OpenCV
        frame, planar B, G, R planes); the streams are those of the R, G, B picture.
        flip: dwtx_encode_view_flip — "y" for bottom-up surfaces, "x" for mirrored ones, "xy", or one of those per window
        (view_flips); the streams are those of `t.flip(...)` of each window, which is never built.
        signed=True: dwtx_encode_view_signed — an int16 tensor (nothing else) whose samples are the signed integers they
        look like: CT slices in Hounsfield units, elevation tiles, residuals; every other keyword keeps its meaning.
        Without it an int16 tensor stays what it has always been here: the carrier of uint16 bytes (torch's uint16 has few
        operators on the device), so that a picture that crosses zero is read as one that jumps by 65535 there.
        base: dwtx_encode_view_delta — a tensor of `t`'s dtype, windows [H,W,C] and number of windows (any strides a view
        takes, its own pitch, grid, planar or interleaved form and step): the streams are those of the integer picture `t - base`, which is never built and
        need not fit any sample type.  Both tensors are only read: `t[1:]` against `t[:-1]` is one call.  Combines with
        stepped, order and signed; not with flip.  The streams' slots are dwtx_encode_bound16's, 8-bit pictures included."""
        order = view_order(order)
        if base is not None:
            v, vb, W, H, Cn, n, step, bstep = self._delta_views(t, base, None, stepped, signed, flip)
            return self._encode_views(v, step, order, None, None, None, None, W, H, n, capacity, out, info,
                                      pair=("dwtx_encode_view_delta", vb, bstep, 1 if signed else 0))
        v, W, H, Cn, n, step = self._view(t, None, stepped, signed=signed)
        flips = view_flips(flip, n)
        return self._encode_views(v, step if stepped else None, order, None, None, flips, 0 if signed else None, W, H, n, capacity, out, info)

    def encode_view_float(self, t, maxval=255, scale=1.0, bias=0.0, capacity=0, out=None, info=None, stepped=False, order="rgb", flip=None,
                          minval=0):
        """dwtx_encode_view_float: encode_view of a float32 / float16 / bfloat16 strided device tensor (the shapes and
        strides encode_view takes, stepped and order="bgr" included).  The picture that is coded is, per sample,
        `(x.float() * scale + bias).round().clamp(0, maxval)` — two float32 roundings, ties to even, NaN -> 0 — and the
        streams are those of encode_device (maxval <= 255) or encode_device16 (above) on that picture; async.  scale,
        bias: a number, or three, per colour R, G, B.  Returns (streams, info) like encode_view.  A tensor that holds no
        floats, a wrong length of scale or bias and values that are not finite raise ValueError before any device call.
        flip: encode_view's keyword.  minval (other than 0): dwtx_encode_view_signed — the clamp is `.clamp(minval, maxval)`,
        -32768 <= minval < maxval <= 32767, and the streams are those of the signed integer picture."""
        order = view_order(order)
        torch = self.torch
        if not hasattr(t, "dtype") or t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"encode_view_float reads float32, float16 or bfloat16 tensors, not {getattr(t, 'dtype', type(t))}")
        fmt = float_format(t.dtype, scale, bias)
        v, W, H, Cn, n, step = self._view(t, int(maxval), stepped, floats=True)
        flips = view_flips(flip, n)
        lo = self._signed_range(False, minval, maxval, floats=True)[0]
        return self._encode_views(v, step, order, fmt, None, flips, lo, W, H, n, capacity, out, info)

    def decode_view(self, streams, lens, into, maxval=None, levels_max=-1, stepped=False, order="rgb", flip=None, signed=False, minval=None,
                    base=None):
        """dwtx_decode_view: device streams [n,stride] + int64 lens -> the windows of the strided device tensor `into`
        ([n,H,W,C] or [bands,cols,H,W,C]), each picture in its window's top-left corner at the size its stream supports;
        nothing else of `into`'s storage is written.  maxval: the deep pictures' (default 65535).  Returns the list of
        DecodeInfo; syncs once.  stepped=True: dwtx_decode_view_step, for the tensors encode_view takes with it; the
        samples between the pixels (an RGBA surface's alpha) are not written either.  order="bgr": dwtx_decode_view_order —
        R and B are written at each other's places.  flip: dwtx_decode_view_flip — "x", "y", "xy" or one of those per window
        (view_flips): each window holds what `.flip(...)` of the unflipped result would, and a reduced picture lies in the
        corner where its pixel (0, 0) lies.
        signed=True: dwtx_decode_view_signed — `into` is an int16 tensor (nothing else) that receives signed samples;
        [minval, maxval] (defaults -32768 and 32767) is the range the pictures were encoded from, what the clamps of a stream
        that was cut short act at.  Without it an int16 tensor is the carrier of uint16 bytes, as for encode_view.
        base: dwtx_decode_view_delta — the streams hold residuals against `base` (encode_view's keyword): each window
        receives `(base + d).clamp(minval, maxval)` with d the decoded residual under the clamps for [-R, R], R = maxval -
        minval; a whole stream gives back the picture exactly.  A window whose stream is unreadable, or cut before its finest
        level, stays as it is (the DecodeInfo says which).  `base=into` decodes in place; otherwise no window of `into` may
        meet one of `base` (view_delta_check).  Not with flip or levels_max."""
        order = view_order(order)
        lo, maxval = self._signed_range(signed, minval, maxval)
        if base is not None:
            v, vb, W, H, Cn, n, step, bstep = self._delta_views(into, base, maxval, stepped, signed, flip, levels_max)
            return self._decode_views(streams, lens, v, step, order, None, None, None, None, None, W, H, n, -1,
                                      pair=("dwtx_decode_view_delta", vb, bstep, 1 if signed else 0, lo if signed else 0))
        v, W, H, Cn, n, step = self._view(into, maxval, stepped, signed=signed)
        flips = view_flips(flip, n)
        return self._decode_views(streams, lens, v, step if stepped else None, order, None, None, None, flips, lo, W, H, n, levels_max)

    # -- delta chains: each picture against its predecessor, the first against a key (dwtx_*_view_chain) ------------------------

    _NOT_IN_CHAINS = {"flip": "the chain calls take no flips", "levels_max": "a coarse residual has no base of its size",
                      "crop": "the chain calls take no crops", "origins": "the chain calls take no crops", "base": "the key is the base of picture 0, "
                      "and every other picture's base is the picture before it", "scale": "the chain calls take integer samples",
                      "bias": "the chain calls take integer samples", "windows": "the chain calls take no window lists"}

    def _chain_views(self, t, key, maxval, stepped, signed, unsupported):
        """The tensors of a chain call -> its two views, or a ValueError before any device call: the keywords of the other view
        calls that a chain does not take, lists, float tensors, a missing key, and a key of another dtype or window shape."""
        torch = self.torch
        for k in unsupported:
            raise ValueError(f"a chain call does not take {k}= ({self._NOT_IN_CHAINS.get(k, 'no view call has that keyword')})")
        if isinstance(t, (list, tuple)):
            raise ValueError("a chain call takes one grid view, not a list of windows")
        if key is None:
            raise ValueError("a chain call needs its key, the base of picture 0")
        for what, x in (("the tensor", t), ("key", key)):
            if not hasattr(x, "dtype") or x.dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
                raise ValueError(f"a chain call takes integer tensors: {what} holds {getattr(x, 'dtype', type(x))}")
        if key.dtype != t.dtype:
            raise ValueError(f"key needs the tensor's dtype {t.dtype}, not {key.dtype}")
        if key.dim() == 3:
            key = key.unsqueeze(0)
        if key.dim() != 4 or key.shape[0] != 1 or tuple(key.shape[-3:]) != tuple(t.shape[-3:]):
            raise ValueError(f"key is one window {tuple(t.shape[-3:])} or (1,) + that (one call is one chain), not shape {tuple(key.shape)}")
        v, W, H, Cn, n, step = self._view(t, maxval, stepped, signed=signed)
        vk, _, _, _, _, kstep = self._view(key, None, stepped, signed=signed)
        return v, vk, W, H, Cn, n, step, kstep

    def encode_view_chain(self, t, key, capacity=0, out=None, info=None, stepped=False, order="rgb", signed=False, **unsupported):
        """dwtx_encode_view_chain: the windows of `t` (any tensor encode_view takes), each against the one before it and window 0
        against `key` — one window [H,W,C] or [1,H,W,C] of `t`'s dtype with any strides a view takes — -> (streams, info) as
        encode_view(t, base=...) gives for those pairs; async.  `frames[1:]` with `frames[0]` as key codes a whole clip.  The
        streams' slots are dwtx_encode_bound16's.  Not with flip, levels_max, float tensors or lists: ValueError."""
        order = view_order(order)
        v, vk, W, H, Cn, n, step, kstep = self._chain_views(t, key, None, stepped, signed, unsupported)
        return self._encode_views(v, step, order, None, None, None, None, W, H, n, capacity, out, info,
                                  pair=("dwtx_encode_view_chain", vk, kstep, 1 if signed else 0))

    def decode_view_chain(self, streams, lens, into, key, maxval=None, stepped=False, order="rgb", signed=False, minval=None, **unsupported):
        """dwtx_decode_view_chain: device streams [n,stride] + int64 lens of a chain's residuals -> the windows of `into`, window i
        receiving `(window i-1 + d_i).clamp(minval, maxval)` and window 0 `(key + d_0).clamp(...)`: what n calls of
        decode_view(..., base=previous window) of one stream each give, in one call.  A window whose stream is unreadable or cut
        before its finest level stays as it is, and the next picture takes what lies there as its base.  key: one window [H,W,C]
        or [1,H,W,C] of `into`'s dtype, disjoint from every window of `into` (view_chain_check); `frames[0]` as key and
        `frames[1:]` as `into` is the layout it is made for.  Returns the list of DecodeInfo; syncs once.  Not with flip,
        levels_max, float tensors or lists: ValueError."""
        order = view_order(order)
        lo, maxval = self._signed_range(signed, minval, maxval)
        v, vk, W, H, Cn, n, step, kstep = self._chain_views(into, key, maxval, stepped, signed, unsupported)
        return self._decode_views(streams, lens, v, step, order, None, None, None, None, None, W, H, n, -1,
                                  pair=("dwtx_decode_view_chain", vk, kstep, 1 if signed else 0, lo if signed else 0))

    # -- clips: chains with their keys inside the stack, many per call (dwtx_*_view_clips) ---------------------------------------

    _NOT_IN_CLIPS = {"flip": "the clips calls take no flips", "levels_max": "the clips calls write whole pictures only",
                     "crop": "the clips calls take no crops", "origins": "the clips calls take no crops", "base": "a link's base is the picture "
                     "before it, inside the stack", "key": "the keys lie inside the stack: a key outside it is encode_view_chain / decode_view_chain",
                     "scale": "the clips calls take integer samples", "bias": "the clips calls take integer samples",
                     "windows": "the clips calls take no window lists"}

    def _clips_view(self, t, period, maxval, stepped, signed, unsupported):
        """The tensor of a clips call -> its view and period, or a ValueError before any device call: the keywords of the other
        view calls that a clip stack does not take, lists, float tensors and a period that is no integer from 1 up."""
        torch = self.torch
        for k in unsupported:
            raise ValueError(f"a clips call does not take {k}= ({self._NOT_IN_CLIPS.get(k, 'no view call has that keyword')})")
        if isinstance(t, (list, tuple)):
            raise ValueError("a clips call takes one grid view, not a list of windows")
        if not hasattr(t, "dtype") or t.dtype in (torch.float32, torch.float16, torch.bfloat16, torch.float64):
            raise ValueError(f"a clips call takes integer tensors: the tensor holds {getattr(t, 'dtype', type(t))}")
        if isinstance(period, bool) or not hasattr(period, "__index__") or int(period) < 1:
            raise ValueError(f"period is the distance between keys, an integer from 1 up (n or more: one clip), not {period!r}")
        return self._view(t, maxval, stepped, signed=signed) + (int(period),)

    def encode_view_clips(self, t, period, capacity=0, out=None, info=None, stepped=False, order="rgb", signed=False, **unsupported):
        """dwtx_encode_view_clips: the windows of `t` (any integer tensor encode_view takes) as a stack of clips: window i with
        i % period == 0 is a key and gets the stream encode_view gives it — an ordinary stream that any reader shows —, every other
        window a link with the stream of encode_view(t[i:i+1], base=t[i-1:i]) -> (streams, info); async, one pass for all n.
        period >= n: one clip with its key at window 0; period == 1: every picture a key; the last clip may be short.  The streams'
        slots are dwtx_encode_bound16's.  Not with flip, levels_max, crops, float tensors, lists or a key outside the stack
        (encode_view_chain): ValueError."""
        order = view_order(order)
        v, W, H, Cn, n, step, period = self._clips_view(t, period, None, stepped, signed, unsupported)
        return self._encode_views(v, step, order, None, None, None, None, W, H, n, capacity, out, info,
                                  clips=(period, 1 if signed else 0))

    def decode_view_clips(self, streams, lens, into, period, maxval=None, stepped=False, order="rgb", signed=False, minval=None, **unsupported):
        """dwtx_decode_view_clips: device streams [n,stride] + int64 lens of a stack of clips (encode_view_clips) -> the windows
        of `into`, as walking them in order gives: a key (window i, i % period == 0) whose stream is readable and supports the
        whole picture receives what decode_view of that stream alone writes, clamps for [minval, maxval] included — one that is
        not stays as it is, a key cut before its finest level too: nothing is written into its corner —, a link what
        decode_view(..., base=window i-1 as it lies in memory) gives; an unreadable or cut link leaves its window, and the next
        link takes what lies there.  Returns the list of DecodeInfo; syncs once.  Not with flip, levels_max, crops, float
        tensors, lists or a key outside the stack (decode_view_chain): ValueError."""
        order = view_order(order)
        lo, maxval = self._signed_range(signed, minval, maxval)
        v, W, H, Cn, n, step, period = self._clips_view(into, period, maxval, stepped, signed, unsupported)
        return self._decode_views(streams, lens, v, step, order, None, None, None, None, None, W, H, n, -1,
                                  clips=(period, 1 if signed else 0, lo if signed else 0))

    _NOT_IN_CLIPS_CROP = {"flip": "the clips calls take no flips", "levels_max": "the clips calls write whole pictures only",
                          "base": "a link's base is the picture before it, inside the stack",
                          "key": "the keys lie inside the stack: a key outside it is decode_view_chain",
                          "windows": "the clips calls take no window lists", "crop": "the crop's size is that of `into`'s windows"}

    def decode_view_clips_crop(self, streams, lens, into, period, size, origins=None, maxval=None, scale=None, bias=None, stepped=False,
                               order="rgb", signed=False, minval=None, **unsupported):
        """dwtx_decode_view_clips_crop: decode_view_clips of a window of each CLIP, and — when `into` is a float32 / float16 /
        bfloat16 tensor — with every sample written as `v * scale + bias` (decode_view_float's two float32 roundings, then the
        dtype): a loader's random crop per clip and its conversion inside the decode.  `into` holds windows of the crop's size
        ([n,ch,cw,C] or [bands,cols,ch,cw,C], any strides decode_view takes), size=(W, H) is the streams' geometry, origins one
        (x0, y0) pair per clip (ceil(n / period) of them), one pair for all, or None for (0, 0): every window of a clip is cut at
        its clip's origin.  Integer tensors: window i receives that window of what decode_view_clips writes, links onto window
        i - 1 as it lies in memory.  Float tensors (scale, bias: a number or three per colour R, G, B; maxval default 255; minval
        as decode_view_float's): a float window cannot be a base, so a break ends the clip — a key that is unreadable or cut
        before its finest level, and every link from the first unreadable or cut one up to the next key, stay as they are; `into`
        is never read.  Returns the list of DecodeInfo; syncs once.  Not with flip, levels_max, lists or a key outside the
        stack, a wrong number of origins, or scale / bias with an integer tensor: ValueError before any device call."""
        order = view_order(order)
        torch = self.torch
        for k in unsupported:
            raise ValueError(f"decode_view_clips_crop does not take {k}= ({self._NOT_IN_CLIPS_CROP.get(k, 'no view call has that keyword')})")
        if isinstance(into, (list, tuple)):
            raise ValueError("a clips call takes one grid view, not a list of windows")
        if isinstance(period, bool) or not hasattr(period, "__index__") or int(period) < 1:
            raise ValueError(f"period is the distance between keys, an integer from 1 up (n or more: one clip), not {period!r}")
        period = int(period)
        W, H = (int(v) for v in size)
        floats = hasattr(into, "dtype") and into.dtype in (torch.float32, torch.float16, torch.bfloat16)
        if not floats and (scale is not None or bias is not None):
            raise ValueError("scale and bias belong to float tensors")
        fmt = float_format(into.dtype, 1.0 if scale is None else scale, 0.0 if bias is None else bias) if floats else None
        if floats and maxval is None:
            maxval = 255
        lo, maxval = self._signed_range(signed, minval, maxval, floats=floats)
        v, cw, ch, Cn, n, step = self._view(into, None if maxval is None else int(maxval), stepped, floats=floats, signed=signed)
        pairs = clip_origins(origins, n, period)
        org = None if pairs is None else (C.c_int * (2 * len(pairs)))(*[c for p in pairs for c in p])
        sgn = 1 if lo is not None else 0   # (a float tensor with a lower bound of its own: the signed range rule)
        return self._decode_views(streams, lens, v, step, order, fmt, (cw, ch, org), None, None, None, W, H, n, -1,
                                  clips=(period, sgn, lo if sgn else 0))

    def decode_view_float(self, streams, lens, into, maxval=255, scale=1.0, bias=0.0, levels_max=-1, stepped=False, order="rgb", flip=None,
                          minval=0):
        """dwtx_decode_view_float: decode_view into a float32 / float16 / bfloat16 strided device tensor `into` (the shapes
        and strides decode_view takes, stepped and order="bgr" included): every sample decode_view would write becomes
        `v * scale + bias` — two float32 roundings, then the tensor's dtype, bit for bit torch's unfused
        `x.float() * scale + bias` (and `.to(dtype)`) of the integer decode — and nothing else of `into`'s storage is
        written.  maxval: what the streams were encoded from (255, or a deep picture's).  scale, bias: a number, or three,
        per colour R, G, B.  Returns the list of DecodeInfo; syncs once.  A wrong dtype, a wrong length of scale or bias
        and values that are not finite raise ValueError before any device call.  flip: decode_view's keyword (a loader's
        per-picture horizontal flip: a sequence of 0 and "x").  minval (other than 0): dwtx_decode_view_signed — the streams
        hold signed pictures of the range [minval, maxval], and v is the signed, clamped integer (a CT slice straight into
        float16 Hounsfield units)."""
        order = view_order(order)
        torch = self.torch
        if not hasattr(into, "dtype") or into.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"decode_view_float writes float32, float16 or bfloat16 tensors, not {getattr(into, 'dtype', type(into))}")
        fmt = float_format(into.dtype, scale, bias)
        v, W, H, Cn, n, step = self._view(into, int(maxval), stepped, floats=True)
        flips = view_flips(flip, n)
        lo = self._signed_range(False, minval, maxval, floats=True)[0]
        return self._decode_views(streams, lens, v, step, order, fmt, None, None, flips, lo, W, H, n, levels_max)

    def decode_view_crop(self, streams, lens, into, size, origins=None, maxval=None, scale=None, bias=None, levels_max=-1, stepped=False,
                         order="rgb", flip=None, signed=False, minval=None):
        """dwtx_decode_view_crop: decode_view — or decode_view_float, when `into` is a float tensor — of a window of each
        picture: `into` holds windows of the crop's size ([n,ch,cw,C] or [bands,cols,ch,cw,C], any strides decode_view takes),
        size=(W, H) is the streams' geometry, origins a sequence of n (x0, y0) pairs, one pair for all, or None for (0, 0).
        Window i receives the picture's samples from (x0_i, y0_i) on, as far as the stream supports them, and nothing else of
        `into`'s storage is written.  scale, bias: float tensors only.  flip: decode_view's keyword — the crop is flipped inside its window.
        signed, minval: decode_view's keywords (int16 tensors), and decode_view_float's minval for float tensors.
        Returns the list of DecodeInfo; syncs once."""
        order = view_order(order)
        torch = self.torch
        W, H = (int(v) for v in size)
        floats = hasattr(into, "dtype") and into.dtype in (torch.float32, torch.float16, torch.bfloat16)
        if not floats and (scale is not None or bias is not None):
            raise ValueError("scale and bias belong to float tensors")
        fmt = float_format(into.dtype, 1.0 if scale is None else scale, 0.0 if bias is None else bias) if floats else None
        if floats and maxval is None:
            maxval = 255
        lo, maxval = self._signed_range(signed, minval, maxval, floats=floats)
        v, cw, ch, Cn, n, step = self._view(into, None if maxval is None else int(maxval), stepped, floats=floats, signed=signed)
        flips = view_flips(flip, n)
        org = self._origins(origins, n)
        return self._decode_views(streams, lens, v, step, order, fmt, (cw, ch, org), None, flips, lo, W, H, n, levels_max)

    # -- window lists: one pointer per picture (dwtx_encode_view_list / dwtx_decode_view_list) ------------------------

    def _view_list(self, windows, maxval, stepped, signed=False):
        """The View (dev NULL), the ctypes array of the windows' pointers and the fields of a list of device tensors [H,W,C]
        (view_list_fields); floats: whether they hold float samples, and then their FloatFormat's dtype."""
        torch = self.torch
        f, ptrs = view_list_fields(windows, stepped)
        t0 = windows[0]
        floats = t0.dtype in (torch.float32, torch.float16, torch.bfloat16)
        if signed and t0.dtype != torch.int16:
            raise ValueError(f"signed=True takes int16 tensors only, not {t0.dtype}")
        if (not floats and t0.dtype not in (torch.uint8, torch.uint16, torch.int16)) or t0.device != self.device:
            raise ValueError("a window list holds uint8, uint16 / int16 or float32 / float16 / bfloat16 tensors [H,W,C] on the context's device")
        if maxval is None:
            maxval = 255 if floats or t0.dtype == torch.uint8 else 65535
        v = View(None, t0.element_size(), f["channels"], int(maxval), 0, f["row_pitch"], 0, 0, f["channel_stride"])
        return v, (C.c_void_p * len(ptrs))(*ptrs), f, floats

    def encode_view_list(self, windows, maxval=None, scale=None, bias=None, capacity=0, out=None, info=None, stepped=False, order="rgb",
                         flip=None, signed=False, minval=None):
        """dwtx_encode_view_list: encode_view — or encode_view_float, when the windows are float tensors — of a sequence of n
        device tensors [H,W,C] that lie wherever they lie: separately allocated pictures, boxes of a frame, tiles in any
        order, permuted [C,H,W] tensors; one shape, one set of strides, one dtype (view_list_fields).  Windows may overlap
        and repeat.  No stack is built: the library reads each window in place.  maxval (float windows: the quantiser's
        clamp, default 255), scale, bias: as for encode_view_float; stepped, order, flip: as for encode_view.  signed: as for
        encode_view (int16 windows); minval: as for encode_view_float (float windows).  Returns (streams, info) like
        encode_view; async."""
        order = view_order(order)
        v, arr, f, floats = self._view_list(windows, maxval, stepped, signed)
        lo = self._signed_range(signed, minval, maxval, floats=floats)[0]
        if not floats and (scale is not None or bias is not None):
            raise ValueError("scale and bias belong to float tensors")
        fmt = float_format(windows[0].dtype, 1.0 if scale is None else scale, 0.0 if bias is None else bias) if floats else None
        flips = view_flips(flip, f["n"])
        if lo is not None and not floats:   # (int16 windows: the source's range is its samples')
            lo = 0
        return self._encode_views(v, f["pixel_step"], order, fmt, arr, flips, lo, f["W"], f["H"], f["n"], capacity, out, info)

    def decode_view_list(self, streams, lens, windows, size=None, origins=None, maxval=None, scale=None, bias=None, levels_max=-1,
                         stepped=False, order="rgb", flip=None, signed=False, minval=None):
        """dwtx_decode_view_list: decode_view_crop into a sequence of n device tensors [H,W,C] that lie wherever they lie (the
        lists encode_view_list takes), which must be provably disjoint (include/dwtx.h).  size=None: whole pictures of the
        windows' size; else size=(W, H) is the streams' geometry, the windows are crops of it and origins their (x0, y0), as for
        decode_view_crop.  Float windows are written as decode_view_float writes them (maxval, scale, bias).  Nothing but
        the windows' samples is written.  flip: decode_view's keyword.  signed, minval: decode_view's keywords (int16 windows),
        and decode_view_float's minval for float windows.  Returns the list of DecodeInfo; syncs once."""
        order = view_order(order)
        torch = self.torch
        floats_ = windows[0].dtype in (torch.float32, torch.float16, torch.bfloat16)
        lo, maxval = self._signed_range(signed, minval, maxval, floats=floats_)
        v, arr, f, floats = self._view_list(windows, maxval, stepped, signed)
        if not floats and (scale is not None or bias is not None):
            raise ValueError("scale and bias belong to float tensors")
        fmt = float_format(windows[0].dtype, 1.0 if scale is None else scale, 0.0 if bias is None else bias) if floats else None
        cw, ch, n = f["W"], f["H"], f["n"]
        flips = view_flips(flip, n)
        W, H = (cw, ch) if size is None else (int(s) for s in size)
        org = self._origins(origins, n)
        return self._decode_views(streams, lens, v, f["pixel_step"], order, fmt, (cw, ch, org), arr, flips, lo, W, H, n, levels_max)
