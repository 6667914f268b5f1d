"""GPU parity of the encoder's VLI-order passes (pack.hip k_gorder and the exact pass k_lut, k_chain_groups,
k_chain_image, k_gorder_exact, with the 64-group layout they give k_bitscan and k_emit).

The fast pass walks the chains started at orders 0 and 31 over every 64-token group; natural pictures make them
meet within a few tokens, so these tests craft gray one-plane pictures whose groups keep them apart
(tests/orders.py): the fast pass then has to resolve a group from its predecessor, and where that chain of
knowledge breaks the image is flagged (dwtx_stream_info.exact_orders) and the exact pass redoes it.  Every stream
must equal the oracle's, bit counts included, and decode back exactly.  The second half forces the exact pass
(the EXACT_ORDERS option) on the goldens and on pictures with many bit planes: the bytes must not change.

Not covered: the thread loops of k_chain_groups (more than 512 groups of 64 chunks) and k_chain_image (more than
1024 such groups): they need more than 134 M tokens in one picture.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import orc
import orders
from test_pack_gpu import SYNTHETIC_CASES, _synthetic_planes

pytestmark = pytest.mark.gpu
G = json.load(open(os.path.join(orc.GOLDEN, "golden.json")))


def encode_check(ctx, lins, W, H, capacity=0):
    """Encode the one-plane pictures `lins` in one batch; every stream, bit count, token count and entry order must
    be the oracle's and the model's.  -> (streams, infos, models)"""
    import torch

    streams, infos = ctx.encode_planes(torch.from_numpy(np.concatenate(lins)).cuda(), W, H, 1, capacity=capacity)
    models = []
    for lin, s, info in zip(lins, streams, infos):
        want, st = orc.encode_lin(lin, W, H, capacity)
        assert s == want
        assert info.exact_orders in (0, 1)
        if not capacity:
            m = orders.order_model(lin, W, H)
            assert info.total_bits == st.total_bits == m.total_bits
            assert info.tokens == len(m.slots)
            assert info.order0 == m.order0
            models.append(m)
    return streams, infos, models


def decode_check(ctx, opts, streams, lins, W, H):
    want = np.concatenate(lins)
    for two in (0, 1):
        opts.set("two_families", two)
        back, dinfos = ctx.decode_planes(streams, W, H, 1)
        assert all(d.status == 0 and not d.truncated for d in dinfos)
        assert (back.cpu().numpy() == want).all()


@pytest.mark.parametrize("case", orders.ALL_UNMET, ids=lambda c: "a%d_t%d" % c)
def test_every_group_unmet(ctx, opts, case):
    """Orders a and a+1 sustained over the whole picture (a = 0..12: escaped runs from a = 10 on, codes with orders
    above 7 on k_emit's general path), around the fast pass's wave of 63 groups, the exact pass's chunks of 4096
    tokens and its groups of 64 chunks."""
    a, nslots = case
    W, H, lin = orders.all_unmet(a, nslots)
    streams, infos, _ = encode_check(ctx, [lin], W, H)
    if nslots > 64 * orders.SUB:
        assert infos[0].exact_orders == 1
    decode_check(ctx, opts, streams, [lin], W, H)


@pytest.mark.parametrize("a", sorted(orders.STRETCH_SHAPE))
def test_stretches_of_unmet_groups_in_one_batch(ctx, opts, a):
    """Stretches of 1..8 unmet groups between groups that meet, early and across the boundaries of the fast pass's
    waves, as one batch: some images are resolved by the fast pass, others flagged, and k_bitscan and k_emit take
    each image's own layout."""
    W, H = orders.STRETCH_SHAPE[a]
    cases = orders.stretches()
    lins = [orders.stretch_plane(a, k, g0, seed=i) for i, (k, g0) in enumerate(cases)]
    streams, infos, models = encode_check(ctx, lins, W, H)
    for (k, g0), m in zip(cases, models):
        assert m.unmet() == list(range(g0, g0 + k))
    flags = {(k, g0): info.exact_orders for (k, g0), info in zip(cases, infos)}
    assert flags[(1, 1)] == 0   # one unmet group early: resolved from its predecessor
    assert 1 in flags.values()
    decode_check(ctx, opts, streams, lins, W, H)


def test_both_outcomes_occur(ctx):
    """Unmet groups are resolved by the fast pass when there are few of them (two or three early in a picture of
    fewer than 4000 tokens) and flagged for the exact pass when there are many (every group of more than 64)."""
    W, H = 1024, 1024
    few = [orders.planes_from_runs(W, H, orders.runs_for_groups(W, H, 3900, groups, a, 5))
           for a, groups in ((0, range(3, 5)), (3, range(3, 6)), (9, range(1, 3)))]
    _, infos, models = encode_check(ctx, few, W, H)
    assert [len(m.unmet()) for m in models] == [2, 3, 2]
    assert [i.exact_orders for i in infos] == [0, 0, 0]
    W, H, many = orders.all_unmet(1, 80 * orders.SUB)
    _, infos, models = encode_check(ctx, [many], W, H)
    assert len(models[0].unmet()) > 64 and infos[0].exact_orders == 1


def test_order_after_the_header(ctx, opts):
    """A root value of 2^30 leaves order 1 after the header: with runs of 6 it holds for the whole picture (the
    entry of the first group comes from the header side, in the fast pass and in k_chain_image), or only until the
    first two groups end."""
    W, H, lins = orders.high_order0_planes()
    streams, infos, _ = encode_check(ctx, lins, W, H)
    assert [i.order0 for i in infos] == [1, 1]
    assert infos[0].exact_orders == 1 and infos[1].exact_orders == 0
    decode_check(ctx, opts, streams, lins, W, H)
    opts.set("exact_orders", 1)
    streams2, infos2, _ = encode_check(ctx, lins, W, H)
    assert streams2 == streams and [i.exact_orders for i in infos2] == [1, 1]


@pytest.mark.parametrize("no_cut", [0, 1])
def test_capacity_cuts_inside_a_flagged_image(ctx, opts, no_cut):
    """CAPACITY inside the first group, at and after a chunk boundary of the exact pass, in the middle and at the
    end: the bytes are the oracle's prefix, with segments dropped by k_cut or everything coded and then clipped."""
    W, H, lin = orders.all_unmet(0, 3 * orders.CHUNK + 100)
    _, infos, (m,) = encode_check(ctx, [lin], W, H)
    assert infos[0].exact_orders == 1
    full = orc.encode_lin(lin, W, H)[0]
    opts.set("no_capacity_cut", no_cut)
    caps = [m.start[10] // 8, m.start[orders.CHUNK] // 8, m.start[orders.CHUNK] // 8 + 1, m.start[2 * orders.CHUNK + 7] // 8,
            len(full) // 2, len(full) - 1, len(full)]
    for cap in caps:
        streams, infos, _ = encode_check(ctx, [lin], W, H, capacity=cap)
        assert streams[0] == full[:cap], cap
        if no_cut:   # everything is coded: still the exact pass's image
            assert infos[0].exact_orders == 1


# ---- the exact pass forced on every image: the same bytes ---------------------------------------------------

@pytest.mark.parametrize("name", sorted(k for k in G if not G[k].get("heavy")))
def test_forced_exact_pass_on_the_goldens(ctx, opts, name):
    """RGB and gray, the 20001- and 32764-wide pictures, the capacity goldens; the 4096x4096 RGB picture has more
    than 512 * 8 chunks of tokens, so k_lut and k_gorder_exact stride over their grids of 512 blocks."""
    import torch
    import dwt_amd

    rec = G[name]
    W, H, Cn = rec["W"], rec["H"], rec["C"]
    if rec["seed"] is None:
        pix = torch.from_numpy(orc.read_pnm(os.path.join(orc.GOLDEN, "smpte.pnm"))[None].copy()).cuda()
    else:
        pix = ctx.synth_pixels(1, H, W, Cn, seed0=rec["seed"], kind=rec["kind"])
    opts.set("exact_orders", 1)
    streams, info = ctx.encode_device(pix, capacity=rec["capacity"])
    inf = dwt_amd.StreamInfo.from_buffer_copy(info[0].cpu().numpy().tobytes())
    assert inf.exact_orders == 1
    data = streams[0, : inf.nbytes].cpu().numpy().tobytes()
    assert len(data) == rec["dwt_len"]
    assert hashlib.sha256(data).hexdigest() == rec["dwt_sha256"]
    if W * H * Cn >= 3 * 4096 * 4096:
        assert inf.tokens > 512 * 8 * orders.CHUNK


def test_forced_exact_pass_on_host_batches_in_parts(ctx, opts):
    opts.set("exact_orders", 1)
    opts.set("part_images", 3)
    n, H, W, Cn = 8, 72, 100, 3
    pix = np.stack([orc.synth(W, H, Cn, 700 + i, i & 1) for i in range(n)])
    streams, stats = ctx.encode(pix)
    for i in range(n):
        want, ost = orc.encode(pix[i])
        assert streams[i] == want
        assert (stats[i].root_bits, stats[i].total_bits) == (ost.root_bits, ost.total_bits)


@pytest.mark.parametrize("case", SYNTHETIC_CASES)
def test_forced_exact_pass_on_many_bit_planes(ctx, opts, case):
    """Up to 16 bit planes, refinement blocks after the break slots, very sparse and dense planes."""
    import torch

    W, H, Cn, bits, density = case
    rng = np.random.default_rng(W * 7 + H + bits)
    lin = _synthetic_planes(rng, W, H, Cn, bits, density)
    want, st = orc.encode_lin(lin, W, H)
    opts.set("exact_orders", 1)
    streams, infos = ctx.encode_planes(torch.from_numpy(lin).cuda(), W, H, Cn)
    assert streams[0] == want
    assert infos[0].total_bits == st.total_bits and infos[0].exact_orders == 1
    for cap in (len(want) // 3, len(want) - 5):
        cut, cinfos = ctx.encode_planes(torch.from_numpy(lin).cuda(), W, H, Cn, capacity=cap)
        assert cut[0] == want[:cap]
