"""Crafted coefficient planes for the encoder's VLI-order passes, and a plain model of the orders they produce
(test infrastructure only, no GPU).

A gray picture (C=1) whose linearised detail coefficients are 0 or +-1 has one bit plane: the schedule
(encode.c:183-221) codes the levels in linear order, each at plane 0, with no refinement bits.  Its token
sequence is the list of zero runs before the ones, plus the final flush (rle.h:58-63, encode.c:221).

From order o a run v leads to o' = max(ilog2(v + 2^o) - 2, 0) (vli.h:67-84).  A run in [6*2^a, 7*2^a) maps
order a to a and order a+1 to a+1, and pulls the chain started at 0 onto a and the one started at 31 onto a+1:
a 64-token group of such runs is one where the encoder's fast pass (pack.hip k_gorder) sees its two chains
never meet.  Runs of 0 let them meet again (16 of them bring any order down to 0).
"""
import numpy as np

import orc

SUB = 64          # tokens per group of the fast order pass (pack.hip SUB)
WAVE_GROUPS = 63  # groups a wave of the fast pass produces (pack.hip FSUBS)
CHUNK = 4096      # tokens per chunk of the exact pass (pack.hip CHUNK)
SUPER = 64 * CHUNK  # tokens per group of chunks of the exact pass (pack.hip GROUP chunks)


def unmet_run(a):
    """[lo, hi) of the runs that keep the 0- and the 31-chain on orders a and a+1."""
    return 6 << a, 7 << a


def _pixels(W, H):
    g = orc.geometry(W, H)
    return [g.pixels[l] for l in range(g.levels + 1)]


def planes_from_runs(W, H, runs, root=None, signs=None):
    """The [1, W*H] int32 linearised plane whose detail tokens are `runs` (then the final flush of what is left).
    `root`: the pixels[0] root values (default zeros); `signs`: +-1 per run (default a fixed mixed pattern)."""
    px = _pixels(W, H)
    runs = np.asarray(runs, dtype=np.int64)
    m = len(runs)
    assert m >= 1 and (runs >= 0).all()
    pos = px[0] + np.cumsum(runs + 1) - 1
    assert pos[-1] < W * H, "the runs do not fit the picture"
    if signs is None:
        signs = np.where((np.arange(m) // 3) % 2, -1, 1)
    lin = np.zeros((1, W * H), dtype=np.int32)
    lin[0, pos] = signs
    if root is not None:
        lin[0, :px[0]] = root
    return lin


def _vli(o, v):
    """-> (bits of v coded at order o, the order after it)"""
    top = (v + (1 << o)).bit_length() - 1
    return 2 * top - o + 1, max(top - 2, 0)


def _step(o, v):
    top = (v + (1 << o)).bit_length() - 1
    return top - 2 if top > 2 else 0


class Model:
    """order0: the order after root values and plane counts; slots: the run of every token slot the encoder lays
    out (a void slot, -1, at every segment's end, then the final flush); entry: the order before every slot;
    start: the stream bit position of every slot's code; met: per 64-slot group, whether the chains started at 0
    and 31 meet in it; total_bits and vli_calls as the oracle's Stats count them (tokens: every put_vli call)."""

    def __init__(self, order0, slots, entry, start, met, total_bits, vli_calls):
        self.order0, self.slots, self.entry, self.start, self.met = order0, slots, entry, start, met
        self.total_bits, self.vli_calls = total_bits, vli_calls

    def unmet(self):
        return [g for g, m in enumerate(self.met) if not m]


def order_model(lin, W, H):
    """Plain restatement of put_vli over a one-plane gray picture's tokens (encode.c:97-110, 177-221)."""
    lin = np.asarray(lin)
    assert lin.shape == (1, W * H)
    px = _pixels(W, H)
    levels = len(px) - 1
    root = [int(x) for x in lin[0, :px[0]]]
    detail = lin[0, px[0]:]
    assert np.abs(detail).max() == 1, "one bit plane: details are 0 or +-1"
    bits, calls, o = 48, 0, 0
    cnt = max(abs(x) for x in root).bit_length()   # encode.c:97-110
    n, o = _vli(o, cnt)
    bits += n
    calls += 1
    if cnt:
        bits += sum(cnt + (x != 0) for x in root)
    n, o = _vli(o, 1)   # the plane count
    bits += n
    calls += 1
    order0 = o
    # the slots: per level (segment) its ones' runs, then its break slot (void: no refinement bits), then the flush
    pos = np.flatnonzero(detail) + px[0]
    runs = np.diff(np.concatenate(([px[0] - 1], pos))) - 1
    lvl = np.searchsorted(px, pos, side="right") - 1
    slots = []
    prev = 0
    for l in range(levels):
        k = int(np.searchsorted(lvl, l, side="right"))
        slots.extend(int(r) for r in runs[prev:k])
        slots.append(-1)
        prev = k
    slots.append(W * H - 1 - int(pos[-1]))
    entry, start = [], []
    for i, v in enumerate(slots):
        entry.append(o)
        start.append(bits)
        if v >= 0:
            n, o = _vli(o, v)
            bits += n + (i < len(slots) - 1)   # a one's sign follows its run; the flush has none
            calls += 1
    met = []
    for g0 in range(0, len(slots), SUB):
        lo, hi = 0, 31
        for v in slots[g0:g0 + SUB]:
            if v >= 0:
                lo, hi = _step(lo, v), _step(hi, v)
        met.append(lo == hi)
    return Model(order0, slots, entry, start, met, bits, calls)


def runs_for_groups(W, H, nslots, unmet, a, seed=0):
    """Runs whose token slots number `nslots` and whose 64-slot groups in the set `unmet` are filled with runs in
    unmet_run(a) (their chains stay apart); every other group is runs of 0 (its chains meet).  The void slots at
    the segment ends are counted as the encoder lays them out."""
    rng = np.random.default_rng(seed)
    px = _pixels(W, H)
    levels = len(px) - 1
    lo, hi = unmet_run(a)
    nruns = nslots - levels - 1
    runs = []
    p, lvl, s = px[0], 0, 0   # next coefficient, its level, slots so far

    def pick(slot):
        return int(rng.integers(lo, hi)) if slot // SUB in unmet else 0

    for _ in range(nruns):
        v = pick(s)
        cross = int(np.searchsorted(px, p + v, side="right")) - 1 - lvl
        if (s + cross) // SUB != s // SUB:
            v = pick(s + cross)
            cross = int(np.searchsorted(px, p + v, side="right")) - 1 - lvl
        runs.append(v)
        s += cross + 1
        lvl += cross
        p += v + 1
    assert p <= W * H, "the runs do not fit the picture"
    return runs


SHAPES = [(256, 256), (512, 512), (1024, 1024), (2048, 1024), (2048, 2048)]


def shape_for(a, nslots):
    """The smallest of SHAPES whose detail coefficients hold `nslots` runs from unmet_run(a)."""
    for W, H in SHAPES:
        if nslots * (7 << a) + (W * H) // 64 < W * H:
            return W, H
    raise ValueError("no picture holds %d runs of %d" % (nslots, 6 << a))


# ---- the constructions the tests share ----------------------------------------------------------------------

# (a, token slots) of the pictures whose groups all stay unmet: fewer slots than one wave of the fast pass, around
# one and a few chunks of the exact pass, and around one group of chunks (k_chain_groups / k_chain_image chain them)
ALL_UNMET = ([(a, 3000) for a in range(8)] + [(8, 2200), (9, 1100), (10, 560), (11, 280), (12, 140)]
             + [(a, n) for a in (0, 2, 5) for n in (4031, 4032, 4033, 4095, 4096, 4097, 3 * CHUNK + 17)]
             + [(0, SUPER - 1), (0, SUPER), (0, SUPER + 1), (0, 299000), (1, SUPER + 4000)])


def all_unmet(a, nslots, seed=0):
    """-> (W, H, lin): every 64-slot group is filled with runs of unmet_run(a)."""
    W, H = shape_for(a, nslots)
    runs = runs_for_groups(W, H, nslots, range(nslots // SUB + 1), a, seed)
    return W, H, planes_from_runs(W, H, runs)


STRETCH_SHAPE = {0: (256, 256), 2: (256, 256), 5: (512, 512), 8: (1024, 1024)}
STRETCH_SLOTS = 140 * SUB


def stretches():
    """(k, g0): a stretch of k unmet groups from group g0 on — early, ending just before and at the last group of
    the fast pass's first wave (group 62, which is also lane 0 of the second wave), across that boundary, from the
    second wave's first group on, and across the second boundary."""
    out = []
    for k in range(1, 9):
        w = WAVE_GROUPS
        for g0 in (1, w - 1 - k, w - k, w - k // 2, w, 2 * w - k // 2):
            if (k, g0) not in out:
                out.append((k, g0))
    return out


def stretch_plane(a, k, g0, seed=0):
    W, H = STRETCH_SHAPE[a]
    return planes_from_runs(W, H, runs_for_groups(W, H, STRETCH_SLOTS, range(g0, g0 + k), a, seed))


def high_order0_planes(W=256, H=256, nslots=5000):
    """Two pictures whose order after the header is 1, not 0 (a root value of 2^30: 31 bits per root value): the
    first has every group unmet with runs of 6 — orders 0 and 1 both stay where they are, so the entry order set by
    the header side holds for the whole picture — the second only its first two groups."""
    px = _pixels(W, H)
    root = np.zeros(px[0], dtype=np.int64)
    root[1] = -(1 << 30)
    root[2:8] = [5, -3, 0, 1 << 20, 7, -1]
    lins = [planes_from_runs(W, H, runs_for_groups(W, H, nslots, groups, 0, 9), root=root)
            for groups in (range(nslots // SUB + 1), range(2))]
    return W, H, lins
