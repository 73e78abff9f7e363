#!/usr/bin/env python3
"""Phases of `krepp index` on a synthetic genome set, built three ways: the default, --gpu-minimizers, and
--gpu-minimizers --gpu-keys (KR_BUILD_TIMING=1 prints the phases; at most 16 threads).

    python scripts/time_build.py [--genomes 64] [--length 2000000] [--threads 16] [--out profiles/build_keys_timing.txt]

The genomes evolve down a random binary tree (krepp_amd.synth), which is also the guide tree, so the key stage sees what a real
build does: keys shared by clades, every pair once per genome.  The three indexes must be the same files; the script checks.
The "key sort + group" lines are the comparison that matters: the host lines are the code the builder had before the key stage
got its device path (one comparison sort of all pairs on one thread, then a walk over the runs)."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from krepp_amd import synth  # noqa: E402

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
FILES = ("cmer", "inc", "crecord", "metadata", "tree", "reflist")


def write_set(td, n, length, seed):
    nwk = synth.yule_newick(n, seed)
    genomes = synth.evolve_genomes(nwk, length, seed)
    tsv = os.path.join(td, "map.tsv")
    with open(tsv, "w") as m:
        for name, seq in genomes.items():
            p = os.path.join(td, name + ".fna")
            with open(p, "wb") as f:  # four contigs, one line each
                for c in range(4):
                    f.write(b">" + f"{name}_c{c}\n".encode() + seq[length * c // 4:length * (c + 1) // 4].tobytes() + b"\n")
            m.write(f"{name}\t{p}\n")
    tree = os.path.join(td, "tree.nwk")
    open(tree, "w").write(nwk)
    return tsv, tree


def build(tsv, tree, out, threads, flags):
    env = dict(os.environ, KR_BUILD_TIMING="1")
    t0 = time.time()
    r = subprocess.run([EXE, "index", "-i", tsv, "-o", out, "-t", tree, "--seed", "3", "--num-threads", str(threads), *flags],
                       capture_output=True, text=True, env=env)
    wall = time.time() - t0
    if r.returncode:
        sys.exit(f"krepp index {' '.join(flags)} failed:\n{r.stderr}")
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("build ")]
    digest = hashlib.sha256()
    for f in FILES:
        digest.update(open(os.path.join(out, f + "-m4r1-frac"), "rb").read())
    return lines, wall, digest.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "build_keys_timing.txt"))
    a = ap.parse_args()
    threads = min(a.threads, 16)
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        t0 = time.time()
        tsv, tree = write_set(td, a.genomes, a.length, seed=11)
        text = [f"krepp index, {a.genomes} synthetic genomes of {a.length} bp (4 contigs each), k 29 w 35 h 13 m 4 r 1 frac, {threads} threads",
                f"(genomes made in {time.time() - t0:.1f} s)", ""]
        digests = []
        for name, flags in (("default", []), ("--gpu-minimizers", ["--gpu-minimizers"]), ("--gpu-minimizers --gpu-keys", ["--gpu-minimizers", "--gpu-keys"])):
            lines, wall, dg = build(tsv, tree, os.path.join(td, "idx_" + str(len(digests))), threads, flags)
            digests.append(dg)
            text += [f"== {name}: wall {wall:.2f} s, files {dg}"] + ["   " + re.sub(r"^build ", "", ln) for ln in lines] + [""]
            print("\n".join(text[-len(lines) - 2:]), flush=True)
        text.append("the three indexes are the same files" if len(set(digests)) == 1 else "THE INDEXES DIFFER")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(text) + "\n")
    print(text[-1])
    return 0 if len(set(digests)) == 1 else 1


if __name__ == "__main__":
    sys.exit(main())
