#!/usr/bin/env python3
"""Pin the crafted decode cases of tests/decode_cases.py in tests/golden/decode_fuzz.json.

Run where the compiled reference exists (after `make -C oracle`):

    python tests/golden/make_decode_fuzz.py

The record holds digests only — per case its name, word size, family, the expected status and
the first 16 hex digits of the SHA-256 of the blob and of the expected output — so the file
stays small; the blobs themselves are rebuilt from the generator's seed by every test run.

Valid families ("ref": "ran"): the reference (oracle.Reference.decode), the CPU oracle and the
numpy decoder of tests/decode_cases.py must give the same bytes with status 0, or this script
stops.  The malformed family is undefined behaviour in the reference (it has no bounds checks
while it parses a blob): those go to the oracle only ("ref": "ub"), whose status is the
specification's.  The word-size-65 blob is valid for the reference and the oracle ("status" 0)
and above the library's bound ("lib_status" = TDT_E_UNSUPPORTED).
"""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle, Reference  # noqa: E402
from tests import decode_cases as dc  # noqa: E402
from tests.support import E_UNSUPPORTED, digest  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent / "decode_fuzz.json"


def main():
    ref, orc = Reference(), Oracle()
    records = []
    for c in dc.all_cases():
        st, out = orc.decode(c.blob)
        rec = dict(name=c.name, ws=c.ws, family=c.family, status=st, blob=digest(c.blob))
        is65 = c.name.endswith("_ws65")
        if c.family != "malformed" or is65:
            rs, rout, err = ref.decode(c.blob, cap=1 << 18)
            assert rs == st == 0, (c.name, rs, st, err)
            assert rout == out, c.name
            if not is65:
                assert dc.numpy_decode(c.blob) == out, c.name
            rec["ref"] = "ran"
        else:
            assert st != 0, c.name
            rec["ref"] = "ub"
        if is65:
            rec["lib_status"] = E_UNSUPPORTED
        if st == 0:
            rec["out"] = digest(out)
        records.append(rec)
    OUT.write_text(json.dumps(dict(
        generator="tests/golden/make_decode_fuzz.py",
        reference="include/psyne/protocol/tdt_compression.hpp via oracle/_ref/libtdt_ref.so",
        seed=dc.SEED, cases=records), indent=0) + "\n")
    print("cases", len(records), "valid", sum(r["family"] != "malformed" for r in records),
          "statuses", sorted({r["status"] for r in records}))


if __name__ == "__main__":
    main()
