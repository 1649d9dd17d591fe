"""The numpy tile model of tests/anyws_tiled_cases.py (per-tile run starts, the scan of first / last /
inner, every tile's pairs at its pair base) against the CPU oracle on the cases the GPU tests use: the
fixtures and the arithmetic are right before a GPU sees them."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import anyws_tiled_cases as tc


@pytest.fixture(scope="module")
def orc():
    return Oracle()


@pytest.mark.parametrize("ws", tc.WIDTHS)
def test_tile_model_agrees_with_the_oracle(orc, ws):
    tile = tc.kernel_tile()
    assert tile % 4096 == 0
    cfg = orc.config(sample_fraction=1.0, word_size=ws)
    for mkind in tc.MAPPINGS:
        mapping = tc.mapping_of(ws, mkind)
        for name, msg in tc.cases_for(ws, mkind, tile):
            n = msg.size
            assert n > tile and n % ws == 0 and n % 4 == 0, (name, n)
            assert 2 <= -(-n // tile) <= 5, (name, n)
            want = orc.encode(msg, cfg=cfg, mapping=mapping)
            assert tc.tile_model(msg, ws, mapping, tile) == want, (ws, mkind, name)
            # a smaller tile cuts the same message at other places: the same blob
            assert tc.tile_model(msg, ws, mapping, 4096) == want, (ws, mkind, name, "4 KiB tiles")


def test_cases_hold_what_they_name():
    """The crossing runs have the lengths they claim, and whole tiles without a run start exist."""
    tile = tc.kernel_tile()
    for ws in tc.WIDTHS:
        for mkind in tc.MAPPINGS:
            mapping = tc.mapping_of(ws, mkind)
            named = dict(tc.cases_for(ws, mkind, tile))
            for s in (0, 1):
                pos = [p for p in range(ws) if mapping[p] == s]
                # crossing: every cap neighbour occurs as a run that contains a tile boundary's stream byte
                crossing = set()
                for name in ("crossing_a", "crossing_b"):
                    msg = named[name]
                    x = msg.reshape(-1, ws)[:, pos].reshape(-1)
                    st = np.flatnonzero(np.concatenate([[True], x[1:] != x[:-1]]))
                    ends = np.concatenate([st[1:], [x.size]])
                    edges = tc.edges_of(msg.size, ws, mapping, s, tile)
                    crossing |= {int(e - b) for b, e in zip(st, ends) if any(b < q < e for q in edges)}
                assert set(tc.CROSSING) <= crossing, (ws, mkind, s, sorted(crossing))
                for name, empty in (("span1", 1), ("span3", 3)):
                    msg = named[name]
                    x = msg.reshape(-1, ws)[:, pos].reshape(-1)
                    st = np.flatnonzero(np.concatenate([[True], x[1:] != x[:-1]]))
                    bounds = [0] + tc.edges_of(msg.size, ws, mapping, s, tile) + [x.size]
                    none = [not ((st >= a) & (st < b)).any() for a, b in zip(bounds, bounds[1:])]
                    assert sum(none) >= empty, (ws, mkind, s, name)
                x = named["constant"].reshape(-1, ws)[:, pos].reshape(-1)
                assert (x == x[0]).all()
