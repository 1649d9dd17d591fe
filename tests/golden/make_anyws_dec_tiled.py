#!/usr/bin/env python3
"""Pin the cases of tests/anyws_dec_tiled_cases.py in tests/golden/anyws_dec_tiled.json.

    python tests/golden/make_anyws_dec_tiled.py

The record holds digests only — per case its name, word size and the first 16 hex digits of the
SHA-256 of the blob and of the expected output; the blobs are rebuilt from the generator's seed by
every test run.  The expected output is the CPU oracle's; the numpy decoder of tests/decode_cases.py
and, where the compiled reference exists (oracle/_ref/, after `make -C oracle`), the reference must
give the same bytes with status 0, or this script stops.  The case whose counts sum past 2^32 is
marked oracle-only: the oracle decodes lazily, the other two would expand 4 GiB.
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle  # noqa: E402
from tests import anyws_dec_tiled_cases as tc  # noqa: E402
from tests.decode_cases import numpy_decode  # noqa: E402
from tests.support import digest  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent / "anyws_dec_tiled.json"


def main():
    orc = Oracle()
    ref = None
    if (ROOT / "oracle" / "_ref" / "libtdt_ref.so").exists():
        from oracle.oracle import Reference
        ref = Reference()
    records = []
    for c in tc.all_cases(with_big=True):
        st, out = orc.decode(c.blob)
        assert st == 0, c.name
        if not c.oracle_only:
            assert numpy_decode(c.blob) == out, c.name
            if ref is not None:
                rs, rout, err = ref.decode(c.blob, cap=1 << 18)
                assert rs == 0 and rout == out, (c.name, rs, err)
        records.append(dict(name=c.name, ws=c.ws, blob=digest(c.blob), out=digest(out), oracle_only=bool(c.oracle_only)))
    OUT.write_text(json.dumps(dict(
        generator="tests/golden/make_anyws_dec_tiled.py",
        reference="the CPU oracle (oracle/tdt_oracle.c)" + ("; compared with oracle/_ref/libtdt_ref.so" if ref else ""),
        seed=tc.SEED, tile=tc.kernel_tile(), block_pairs=tc.block_pairs(), cases=records), indent=0) + "\n")
    print("cases", len(records), "reference", "compared" if ref else "absent")


if __name__ == "__main__":
    main()
