"""A frame too big (or too awkward) to code whole, as tiles: dwtx_tile_groups cuts it into at most four groups of
same-geometry tiles, and each group is one strided view of the frame — one encode_view / decode_view call per group,
no tile is copied.  A tiled frame is the groups' ordinary .dwt streams plus the plan (frame size and `tile`), which
the caller keeps, like maxval: there is no container format."""
from . import tile_groups


def group_view(frame, g):
    """The tiles of group g (TileGroup) of a device tensor frame [H,W,C], as a strided tensor [rows,cols,g.H,g.W,C].  The
    frame's own strides are kept: a planar frame, `chw.permute(1, 2, 0)`, gives planar tiles."""
    if frame.dim() != 3:
        raise ValueError("a frame is a tensor [H,W,C]")
    sh, sw, sc = frame.stride()
    return frame.as_strided((g.rows, g.cols, g.H, g.W, frame.shape[2]), (g.H * sh, g.W * sw, sh, sw, sc),
                            frame.storage_offset() + g.y0 * sh + g.x0 * sw)


def encode_frame(ctx, frame, tile, capacity=0, stepped=False, order="rgb"):
    """frame: device tensor [H,W,C] (uint8, or uint16 / int16; interleaved, or a planar [C,H,W] frame permuted) -> one (TileGroup, streams, lens, info) per group of
    tile_groups(W, H, tile); a group's stream i is its tile (i // cols, i % cols).  Async, like encode_view.
    stepped: encode_view's keyword — the frame may be `rgba[..., :3]` or `rgba[..., 3:]` of an RGBA surface [H,W,4].
    order: encode_view's keyword — "bgr" for `bgra[..., :3]` of a BGRA surface, or a BGR frame."""
    out = []
    for g in tile_groups(frame.shape[1], frame.shape[0], tile):
        streams, info = ctx.encode_view(group_view(frame, g), capacity, stepped=stepped, order=order)
        out.append((g, streams, ctx.stream_lengths(info), info))
    return out


def decode_frame(ctx, groups, into, maxval=None, levels_max=-1, stepped=False, order="rgb"):
    """groups: what encode_frame returned (or (TileGroup, streams, lens) triples) -> every tile decoded in place in the
    device tensor `into` [H,W,C]; a tile whose stream was cut comes out reduced in its own corner.  Returns the lists of
    DecodeInfo, one per group.  stepped, order: decode_view's keywords."""
    return [ctx.decode_view(g[1], g[2], group_view(into, g[0]), maxval, levels_max, stepped=stepped, order=order) for g in groups]
