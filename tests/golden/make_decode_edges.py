#!/usr/bin/env python3
"""Pin the decode edge cases of tests/decode_edge_cases.py in tests/golden/decode_edges.json.

Run where the compiled reference exists (after `make -C oracle`):

    python tests/golden/make_decode_edges.py

The record holds digests only — per case its name, word size, family and the first 16 hex digits
of the SHA-256 of the blob and of the expected output; the blobs themselves are rebuilt from the
generator's seed by every test run.  Every case is a valid blob: the reference
(oracle.Reference.decode), the CPU oracle and the numpy decoder of tests/decode_cases.py must give
the same bytes with status 0, or this script stops.  "dropped" lists cases left out because the
three disagree; it must stay empty (a disagreement is a finding to write up, not to hide).
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle, Reference  # noqa: E402
from tests import decode_edge_cases as ec  # noqa: E402
from tests.support import digest  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent / "decode_edges.json"


def main():
    ref, orc = Reference(), Oracle()
    records = []
    for c in ec.all_cases():
        st, out = orc.decode(c.blob)
        rs, rout, err = ref.decode(c.blob, cap=1 << 18)
        assert rs == st == 0, (c.name, rs, st, err)
        assert rout == out, c.name
        assert ec.numpy_decode(c.blob) == out, c.name
        records.append(dict(name=c.name, ws=c.ws, family=c.family, blob=digest(c.blob), out=digest(out)))
    OUT.write_text(json.dumps(dict(
        generator="tests/golden/make_decode_edges.py",
        reference="include/psyne/protocol/tdt_compression.hpp via oracle/_ref/libtdt_ref.so",
        seed=ec.SEED, geometry=ec.geometry(), dropped=[], cases=records), indent=0) + "\n")
    print("cases", len(records), "decoded bytes", sum(ec.parse(c.blob)[0] for c in ec.all_cases()))


if __name__ == "__main__":
    main()
