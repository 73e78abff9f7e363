#!/usr/bin/env python3
"""Writes tests/golden/llh_mp.npy: the likelihood objective in 256-bit arithmetic (tests/llh_mp.py) on seeded cases -- the inputs,
f rounded to double, the error unit B, and for the minimised cases d*, B(d*) and f at d*, d* +- w, d* +- 2w.
Needs mpmath and numpy only (no reference, no oracle, no GPU); a few minutes on a handful of cores.  Every case is seeded by its own
key, so the output does not depend on how the work is spread."""
import os
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import llh_mp  # noqa: E402


def main():
    keys = llh_mp.case_keys()
    with Pool(min(16, os.cpu_count() or 1)) as pool:
        rows = pool.map(llh_mp.make_case, keys, chunksize=8)
    llh_mp.save_rows(rows)
    print(f"{len(rows)} cases, {sum(int(r[0]) % 10 for r in rows)} minimised, {os.path.getsize(llh_mp.FIXTURE)} bytes")


if __name__ == "__main__":
    main()
