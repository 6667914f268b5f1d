"""CPU tests: the VLI-order model of tests/orders.py against the oracle's entropy stage, and the crafted planes of
the encoder's order-pass tests (tests/test_orders_gpu.py) checked to have the unmet groups they are meant to have."""
import numpy as np
import pytest

import orc
import orders


def check_on_oracle(lin, W, H):
    m = orders.order_model(lin, W, H)
    _, st = orc.encode_lin(lin, W, H)
    assert m.total_bits == st.total_bits
    assert m.vli_calls == st.tokens   # every put_vli call: root counts and plane counts included
    assert m.start[-1] + orders._vli(m.entry[-1], m.slots[-1])[0] == st.total_bits
    return m


def test_unmet_runs_keep_the_chains_apart():
    for a in range(20):
        lo, hi = orders.unmet_run(a)
        for v in (lo, (lo + hi) // 2, hi - 1):
            assert orders._step(a, v) == a and orders._step(a + 1, v) == a + 1
            assert orders._step(0, v) == a
            o = 31
            for _ in range(16):
                o = orders._step(o, v)
            assert o == a + 1
        assert orders._step(a, hi) != a or orders._step(a + 1, hi) != a + 1   # the range is tight above


@pytest.mark.parametrize("seed", range(6))
def test_model_on_random_runs(seed):
    """Runs of every size (zeros, small ones, escaped ones) and root values of every width."""
    rng = np.random.default_rng(seed)
    W, H = [(64, 64), (131, 77), (256, 256), (300, 17), (512, 512), (1000, 9)][seed]
    g = orc.geometry(W, H)
    n = W * H - g.pixels[0]
    runs = rng.geometric(rng.uniform(0.001, 0.7), n) - 1
    runs[rng.integers(10, 50, 3)] = [4095, 5000, n // 3]   # escaped runs, where they fit
    runs = runs[:np.searchsorted(np.cumsum(runs + 1), n - 1)]
    root = rng.integers(-(1 << int(rng.integers(0, 31))), 1 << int(rng.integers(0, 31)), g.pixels[0])
    lin = orders.planes_from_runs(W, H, runs, root=root)
    m = check_on_oracle(lin, W, H)
    assert len(m.slots) == len(runs) + g.levels + 1


@pytest.mark.parametrize("case", orders.ALL_UNMET, ids=lambda c: "a%d_t%d" % c)
def test_all_unmet_planes(case):
    a, nslots = case
    W, H, lin = orders.all_unmet(a, nslots)
    m = check_on_oracle(lin, W, H)
    assert len(m.slots) == nslots
    assert all(not met for met in m.met[:-1])   # (the last group ends with the flush of the picture's tail)
    i0 = next(i for i, v in enumerate(m.slots) if v >= 0)   # (before the first token: the order after the header)
    assert set(m.entry[i0 + 1:-1]) <= {a, a + 1}


@pytest.mark.parametrize("a", sorted(orders.STRETCH_SHAPE))
def test_stretch_planes(a):
    W, H = orders.STRETCH_SHAPE[a]
    for k, g0 in orders.stretches():
        lin = orders.stretch_plane(a, k, g0)
        m = orders.order_model(lin, W, H)
        assert len(m.slots) == orders.STRETCH_SLOTS
        assert m.unmet() == list(range(g0, g0 + k)), (k, g0)
    for k, g0 in [(1, 1), (4, 63 - 2), (8, 126 - 4)]:
        check_on_oracle(orders.stretch_plane(a, k, g0), W, H)


def test_high_order0_planes():
    W, H, lins = orders.high_order0_planes()
    ms = [check_on_oracle(lin, W, H) for lin in lins]
    assert [m.order0 for m in ms] == [1, 1]
    assert set(ms[0].entry[:-1]) == {1}   # the header's order holds all the way
    assert len(ms[0].unmet()) >= 64 and ms[1].unmet()[:2] == [0, 1] and ms[1].met[2]
