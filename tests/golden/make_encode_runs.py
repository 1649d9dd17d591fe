#!/usr/bin/env python3
"""Pin the run-structured encode cases of tests/encode_run_cases.py in tests/golden/encode_runs.json.

Run where the compiled reference exists (after `make -C oracle`):

    python tests/golden/make_encode_runs.py

The record holds digests only — per case its name, word size, mapping, size, family and the first
16 hex digits of the SHA-256 of the message and of the blob; the messages are rebuilt from the
generator's seed by every test run.

The script stops unless, for every case, the reference (oracle.Reference.encode) and the CPU oracle
give the same blob with sample_fraction = 1.0 at bandwidth 10, the blob is a TDT blob, and the
oracle decodes it back to the message.  The cases' premise is that the analysed mapping is the
intended one: a case where it is not is dropped and listed by name under "dropped"; more than
PREMISE_CAP of a width's cases dropped stops the script too.
"""
from __future__ import annotations

import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle, Reference  # noqa: E402
from tests import encode_run_cases as ec  # noqa: E402
from tests.support import digest  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent / "encode_runs.json"
PREMISE_CAP = 0.02


def main():
    ref, orc = Reference(), Oracle()
    records, dropped, per_width = [], [], {}
    for c in ec.all_cases():
        blob = orc.encode(c.message, cfg=orc.config(word_size=c.ws, sample_fraction=1.0), bandwidth=10.0)
        assert ref.encode(c.message, sample_fraction=1.0, word_size=c.ws, bandwidth=10.0) == blob, c.name
        assert blob[:4] == b"DTDT", c.name
        st, back = orc.decode(blob)
        assert st == 0 and back == c.message.tobytes(), c.name
        per_width[c.ws] = per_width.get(c.ws, 0) + 1
        if tuple(int(m) for m in np.frombuffer(blob[20:20 + 4 * c.ws], np.int32)) != tuple(c.mapping):
            dropped.append(c.name)
            continue
        records.append(dict(name=c.name, ws=c.ws, mapping="".join(str(m) for m in c.mapping), n=c.n, family=c.family,
                            message=digest(c.message.tobytes()), blob=digest(blob)))
    for ws, total in per_width.items():
        gone = sum(1 for name in dropped if name.startswith("ws%d_" % ws))
        assert gone <= PREMISE_CAP * total, "width %d: %d of %d cases miss the intended mapping" % (ws, gone, total)
    ec.check_coverage([c for c in ec.all_cases() if c.name not in dropped])
    OUT.write_text(json.dumps(dict(
        generator="tests/golden/make_encode_runs.py",
        reference="include/psyne/protocol/tdt_compression.hpp via oracle/_ref/libtdt_ref.so",
        seed=ec.SEED, dropped=dropped, cases=records), indent=0) + "\n")
    print("cases", len(records), "dropped", len(dropped), "bytes", sum(r["n"] for r in records),
          "per width", dict(sorted(per_width.items())))


if __name__ == "__main__":
    main()
