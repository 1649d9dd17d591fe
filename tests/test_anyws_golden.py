"""The CPU oracle against the generic-word-size fixtures (tests/golden/make_anyws.py: word sizes
3, 5, 6, 7, 12, 24, 32, 40 and 64 through the compiled reference).  Pins the yardstick the GPU
tests of those widths (tests/test_gpu_anyws.py) compare with."""
import struct

import numpy as np
import pytest

from oracle.oracle import Oracle, Reference
from tests.anyws_cases import WIDTHS, intended_mapping, load_anyws


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


@pytest.fixture(scope="module")
def cases():
    return load_anyws()


def test_fixture_has_every_family_and_width(cases):
    for fam in ("constructed", "same", "equal", "uniform"):
        assert {c.ws for c in cases if c.family == fam} == set(WIDTHS), fam
    assert sum(c.family == "uncp" for c in cases) == 2
    names = {c.name for c in cases if c.op == "decode"}
    for n in ("four_streams_ws12", "short_stream_ws12", "odd_trailing_byte_ws12", "count_zero_pairs_ws12",
              "orig_tail_bytes_ws12", "truncated_stream_ws12", "mapping_range_ws12", "ws65"):
        assert n in names


def test_oracle_reproduces_every_blob(oracle, cases):
    n = 0
    for c in cases:
        if c.op != "encode":
            continue
        cfg = oracle.config(word_size=c.ws, sample_fraction=c.sample_fraction, min_tensor_size=c.min_tensor)
        assert oracle.encode(c.input, cfg=cfg, bandwidth=c.bandwidth, cpu=c.cpu) == c.expected.tobytes(), c.name
        st, back = oracle.decode(c.expected)
        assert st == 0 and back == c.input.tobytes(), c.name
        n += 1
    assert n == 4 * len(WIDTHS) + 2


def test_constructed_mapping_and_shapes(oracle, cases):
    for c in cases:
        if c.family == "constructed":
            _, _, mp = oracle.analyze(c.input, word_size=c.ws)
            assert list(mp) == intended_mapping(c.ws) == c.mapping, c.name
            assert c.input.size >= 1024 and (c.input.size // c.ws) % 4 == 0
            assert struct.unpack_from("<I", c.expected.tobytes(), 8)[0] == 2
        elif c.family == "same":
            assert struct.unpack_from("<I", c.expected.tobytes(), 8)[0] == 1  # num_streams
        elif c.family == "uncp":
            assert c.expected.tobytes()[:4] == b"PCNU" and c.expected.size == c.input.size + 4


def test_oracle_reproduces_every_decode(oracle, cases):
    for c in cases:
        if c.op != "decode":
            continue
        st, out = oracle.decode(c.input)
        assert st == c.status, (c.name, st)
        if st == 0:
            assert out == c.expected.tobytes(), c.name
    by = {c.name: c for c in cases}
    assert by["truncated_stream_ws12"].status == 3 and by["mapping_range_ws12"].status == 4
    assert by["ws65"].status == 0 and by["ws65"].lib_status == 6


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref not built (needs the reference at build time)")
def test_oracle_vs_reference_random_widths():
    o, r = Oracle(), Reference()
    rng = np.random.default_rng(77)
    for k in range(60):
        ws = WIDTHS[k % len(WIDTHS)]
        wc = int(rng.integers(64, 400)) * 4
        if k % 3 == 0:
            d = rng.integers(0, 256, wc * ws, dtype=np.uint8)
        elif k % 3 == 1:
            d = rng.integers(0, 3, (wc, ws), dtype=np.uint8)
            d[:, ::2] = rng.integers(0, 256, (wc, (ws + 1) // 2), dtype=np.uint8)
            d = d.reshape(-1)
        else:
            vals = []
            while len(vals) < wc * ws:
                vals += [int(rng.integers(0, 4))] * int(rng.integers(1, 700))
            d = np.array(vals[: wc * ws], np.uint8)
        assert o.encode(d, cfg=o.config(word_size=ws)) == r.encode(d, word_size=ws), (k, ws)
