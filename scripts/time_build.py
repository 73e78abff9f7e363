#!/usr/bin/env python3
"""Phases of `krepp index` on a synthetic genome set, built four ways: the default, --gpu-minimizers,
--gpu-minimizers --gpu-keys and --gpu-colours (KR_BUILD_TIMING=1 prints the phases; at most 16 threads).

    python scripts/time_build.py [--genomes 64] [--length 2000000] [--threads 16] [--out profiles/build_keys_timing.txt]
                                 [--only NAME,...] [--repeat R] [--baseline-exe PATH] [--append]

The genomes evolve down a random binary tree (krepp_amd.synth), which is also the guide tree, so the key stage sees what a real
build does: keys shared by clades, every pair once per genome.  All indexes must be the same files; the script checks.
The "key sort + group" lines are the comparison that matters for --gpu-keys: the host lines are the code the builder had before
the key stage got its device path (one comparison sort of all pairs on one thread, then a walk over the runs).  For --gpu-colours
it is "colour classes" + "colours" against the "colours" line of --gpu-minimizers --gpu-keys, whose loop folds every group.
--only: the ways to build, by name (default, --gpu-minimizers, --gpu-keys, --gpu-colours); --repeat: every way R times;
--baseline-exe: another build of the CLI (an earlier commit's), run with --gpu-minimizers --gpu-keys on the same genomes in the
same session; --append: add to the file instead of replacing it."""
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
WAYS = (("default", "default", []), ("--gpu-minimizers", "--gpu-minimizers", ["--gpu-minimizers"]),
        ("--gpu-keys", "--gpu-minimizers --gpu-keys", ["--gpu-minimizers", "--gpu-keys"]), ("--gpu-colours", "--gpu-colours", ["--gpu-colours"]))


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


def build(exe, tsv, tree, out, threads, flags):
    env = dict(os.environ, KR_BUILD_TIMING="1")
    t0 = time.time()
    r = subprocess.run([exe, "index", "-i", tsv, "-o", out, "-t", tree, "--seed", "3", "--num-threads", str(threads), *flags],
                       capture_output=True, text=True, env=env, timeout=600)
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
    ap.add_argument("--only", default=",".join(w[0] for w in WAYS))
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--baseline-exe", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    threads = min(a.threads, 16)
    runs = [(name, EXE, flags) for key, name, flags in WAYS if key in a.only.split(",")]
    if a.baseline_exe:
        runs.insert(0, ("baseline build, --gpu-minimizers --gpu-keys", a.baseline_exe, ["--gpu-minimizers", "--gpu-keys"]))
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as td:
        t0 = time.time()
        tsv, tree = write_set(td, a.genomes, a.length, seed=11)
        text = [f"krepp index, {a.genomes} synthetic genomes of {a.length} bp (4 contigs each), k 29 w 35 h 13 m 4 r 1 frac, {threads} threads",
                f"(genomes made in {time.time() - t0:.1f} s)", ""]
        digests = []
        for name, exe, flags in runs:
            for rep in range(a.repeat):
                lines, wall, dg = build(exe, tsv, tree, os.path.join(td, "idx"), threads, flags)  # (every run over the last one's files)
                digests.append(dg)
                run = f" (run {rep + 1} of {a.repeat})" if a.repeat > 1 else ""
                text += [f"== {name}{run}: wall {wall:.2f} s, files {dg}"] + ["   " + re.sub(r"^build ", "", ln) for ln in lines] + [""]
                print("\n".join(text[-len(lines) - 2:]), flush=True)
        text.append(f"the {len(digests)} indexes are the same files" if len(set(digests)) == 1 else "THE INDEXES DIFFER")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "a" if a.append else "w").write(("\n" if a.append else "") + "\n".join(text) + "\n")
    print(text[-1])
    return 0 if len(set(digests)) == 1 else 1


if __name__ == "__main__":
    sys.exit(main())
