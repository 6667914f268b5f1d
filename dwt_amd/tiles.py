"""A frame too big (or too awkward) to code whole, as tiles: dwtx_tile_groups cuts it into at most four groups of
same-geometry tiles, and each group is one strided view of the frame — one encode_view / decode_view call per group,
no tile is copied.  A tiled frame is the groups' ordinary .dwt streams plus the plan (frame size and `tile`), which
the caller keeps, like maxval: there is no container format."""
from . import tile_groups, view_flips


def group_view(frame, g):
    """The tiles of group g (TileGroup) of a device tensor frame [H,W,C], as a strided tensor [rows,cols,g.H,g.W,C].  The
    frame's own strides are kept: a planar frame, `chw.permute(1, 2, 0)`, gives planar tiles."""
    if frame.dim() != 3:
        raise ValueError("a frame is a tensor [H,W,C]")
    sh, sw, sc = frame.stride()
    return frame.as_strided((g.rows, g.cols, g.H, g.W, frame.shape[2]), (g.H * sh, g.W * sw, sh, sw, sc),
                            frame.storage_offset() + g.y0 * sh + g.x0 * sw)


def group_windows(frame, g, flip):
    """The tiles of group g of the UPRIGHT picture of a bottom-up and / or mirrored frame [H,W,C] (flip: the mask 1..3 of
    view_flips), as a list of rows * cols slices of the frame in PICTURE order: entry i is tile (i // cols, i % cols) of
    the upright frame, which lies mirrored in memory — the window list the flipped calls take."""
    if frame.dim() != 3:
        raise ValueError("a frame is a tensor [H,W,C]")
    H, W = frame.shape[0], frame.shape[1]
    out = []
    for r in range(g.rows):
        y = g.y0 + r * g.H
        y = H - y - g.H if flip & 2 else y
        for c in range(g.cols):
            x = g.x0 + c * g.W
            x = W - x - g.W if flip & 1 else x
            out.append(frame[y:y + g.H, x:x + g.W])
    return out


def _frame_flip(flip):
    f = view_flips(flip, 1)
    if f is not None and f[1] is not None:
        raise ValueError("a frame has one flip: None, 'x', 'y' or 'xy'")
    return f[0] if f else 0


def encode_frame(ctx, frame, tile, capacity=0, stepped=False, order="rgb", flip=None, base=None):
    """frame: device tensor [H,W,C] (uint8, or uint16 / int16; interleaved, or a planar [C,H,W] frame permuted) -> one (TileGroup, streams, lens, info) per group of
    tile_groups(W, H, tile); a group's stream i is its tile (i // cols, i % cols).  Async, like encode_view.
    stepped: encode_view's keyword — the frame may be `rgba[..., :3]` or `rgba[..., 3:]` of an RGBA surface [H,W,4].
    order: encode_view's keyword — "bgr" for `bgra[..., :3]` of a BGRA surface, or a BGR frame.
    flip: "y" for a bottom-up frame, "x" for a mirrored one, "xy": the streams are those of encode_frame of the upright
    frame, `frame.flip(...)`, tile for tile — each group travels as a window list in picture order (group_windows).
    base: encode_view's keyword — a frame of the same shape and dtype; every tile is coded against the same tile of it."""
    out = []
    f = _frame_flip(flip)
    _check_base(frame, base, f)
    for g in tile_groups(frame.shape[1], frame.shape[0], tile):
        if base is not None:
            streams, info = ctx.encode_view(group_view(frame, g), capacity, stepped=stepped, order=order, base=group_view(base, g))
        elif f:
            streams, info = ctx.encode_view_list(group_windows(frame, g, f), capacity=capacity, stepped=stepped, order=order, flip=f)
        else:
            streams, info = ctx.encode_view(group_view(frame, g), capacity, stepped=stepped, order=order)
        out.append((g, streams, ctx.stream_lengths(info), info))
    return out


def _check_base(frame, base, flip):
    if base is None:
        return
    if flip:
        raise ValueError("base= does not combine with flip")
    if tuple(base.shape) != tuple(frame.shape) or base.dtype != frame.dtype:
        raise ValueError(f"base= needs a frame of shape {tuple(frame.shape)} and dtype {frame.dtype}, not {tuple(base.shape)} {base.dtype}")


def decode_frame(ctx, groups, into, maxval=None, levels_max=-1, stepped=False, order="rgb", flip=None, base=None):
    """groups: what encode_frame returned (or (TileGroup, streams, lens) triples) -> every tile decoded in place in the
    device tensor `into` [H,W,C]; a tile whose stream was cut comes out reduced in its own corner.  Returns the lists of
    DecodeInfo, one per group.  stepped, order: decode_view's keywords.  flip: encode_frame's keyword — `into` receives the
    bottom-up and / or mirrored frame; a reduced tile lies in the corner of its window where its pixel (0, 0) lies.
    base: decode_view's keyword — the frame the tiles were coded against (`base=into` decodes in place); a tile whose stream
    was cut before its finest level stays as it is."""
    f = _frame_flip(flip)
    _check_base(into, base, f)
    if base is not None:
        return [ctx.decode_view(g[1], g[2], group_view(into, g[0]), maxval, levels_max, stepped=stepped, order=order, base=group_view(base, g[0]))
                for g in groups]
    if f:
        return [ctx.decode_view_list(g[1], g[2], group_windows(into, g[0], f), maxval=maxval, levels_max=levels_max, stepped=stepped, order=order,
                                     flip=f) for g in groups]
    return [ctx.decode_view(g[1], g[2], group_view(into, g[0]), maxval, levels_max, stepped=stepped, order=order) for g in groups]
