#!/usr/bin/env python3
"""Record tests/golden/search_bits.npz on one MI355X: the score bits and ids of every case of
tests/search_bits_cases.py, from whichever build of the library is loaded (``HIPZAP_LIB`` selects another one).
The file holds outputs only and its bytes depend on the arrays alone, so two builds that compute the same bits
write identical files.

    python scripts/search_bits_record.py [--out tests/golden/search_bits.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import search_bits_cases as B  # noqa: E402


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "tests", "golden", "search_bits.npz")
    arrays = {}
    for name in B.NAMES:
        arrays[name + "_scores"], arrays[name + "_ids"] = B.run_case(name)
        print(name, "ok", flush=True)
    B.save_fixture(out, arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
