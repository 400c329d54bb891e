"""Record tests/golden/decode_refusals.json: the exception type and message of every single illegal
combination in tests/test_decode_plumbing.py's ``VIOLATIONS``, through every door that takes its
arguments (``Decoder``, ``generate_cached``, ``cached_decoder``, ``generate_batch``, ``batch_decoder``).

The fixture pins what the decode runtime refuses across changes of its Python, so it is recorded with
the ``nanosandbox_amd/runtime/decode.py`` of the commit to compare against and never with the tree
under test.  No GPU is needed:

    python scripts/record_decode_refusals.py [--out PATH]

Nothing is written if any case goes through.
"""

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_decode_plumbing as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=G.GOLDEN)
    a = ap.parse_args()
    print(f"decode runtime: {G.decode.__file__}", flush=True)
    model = G.build_model()
    cases, through = {}, []
    for name, doors in G.VIOLATIONS.items():
        cases[name] = {door: G.refusal(model, door, kw) for door, kw in doors.items()}
        through += [f"{name} through {door}" for door, got in cases[name].items() if got is None]
        for door, got in cases[name].items():
            print(f"{name} / {door}: {got}", flush=True)
    if through:
        sys.exit("not refused, nothing written: " + "; ".join(through))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"model": G.ARGS, "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
