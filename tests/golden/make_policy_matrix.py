#!/usr/bin/env python3
"""Pin the routing cases of tests/policy_cases.py in tests/golden/policy_matrix.json.

Run where the compiled reference exists (after `make -C oracle`):

    python tests/golden/make_policy_matrix.py

Per case the record holds what the compiled reference (oracle.Reference.policy: one object configured
with the case's width, min_tensor_size and both thresholds, and fed its metrics) answers:

    st    should_transform's answer (1 / 0)
    tdt   1 when encode's output starts with the TDT magic, 0 for the UNCP marker
    len   the output's length
    sha   the first 16 hex digits of its SHA-256

and no message bytes: every test run rebuilds the messages from the generator's seed.  The reference
takes every width of the cases, the generic ones (3, 12, 40) included: none is pinned by the C oracle
alone.  The script stops unless the CPU oracle gives the same answer and the same blob for every case,
`st` and `tdt` are what policy_cases.predicate / compresses say, and the premises about the content
hold (policy_cases.check_blob_lengths)."""
from __future__ import annotations

import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from oracle.oracle import Oracle, Reference  # noqa: E402
from tests import policy_cases as pc  # noqa: E402
from tests.support import digest  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent / "policy_matrix.json"


def main():
    ref, orc = Reference(), Oracle()
    cases = pc.all_cases()
    pc.check_coverage(cases)
    records, lengths = [], {}
    for c in cases:
        st, blob = ref.policy(c.message, word_size=c.ws, bandwidth=c.bandwidth, cpu=c.cpu, min_tensor_size=c.min_tensor,
                              bandwidth_threshold_mbps=c.bandwidth_threshold, cpu_usage_threshold=c.cpu_threshold)
        cfg = orc.config(word_size=c.ws, sample_fraction=1.0, bandwidth_threshold_mbps=c.bandwidth_threshold,
                         cpu_usage_threshold=c.cpu_threshold, min_tensor_size=c.min_tensor)
        assert orc.encode(c.message, cfg=cfg, bandwidth=c.bandwidth, cpu=c.cpu) == blob, c.name
        assert orc.should_transform(c.n, cfg=cfg, bandwidth=c.bandwidth, cpu=c.cpu) == st, c.name
        assert blob[:4] in (b"DTDT", b"PCNU"), c.name
        tdt = blob[:4] == b"DTDT"
        assert st == pc.predicate(c.n, *c[3:8]) and tdt == pc.compresses(c.ws, c.n, *c[3:8]) == (c.side == "on"), c.name
        lengths[c.name] = len(blob)
        records.append({"name": c.name, "st": int(st), "tdt": int(tdt), "len": len(blob), "sha": digest(blob)})
    pc.check_blob_lengths(cases, lengths)
    OUT.write_text(json.dumps(dict(
        generator="tests/golden/make_policy_matrix.py",
        reference="include/psyne/protocol/tdt_compression.hpp via oracle/_ref/libtdt_ref.so",
        seed=pc.SEED, cases=records), indent=0) + "\n")
    print("cases", len(records), "tdt", sum(r["tdt"] for r in records), "bytes", sum(c.n for c in cases),
          "file", OUT.stat().st_size)


if __name__ == "__main__":
    main()
