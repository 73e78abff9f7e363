"""kr_buf.h, the owning type of every grow-on-demand device / pinned buffer, on the CPU: tests/buf_check.cpp (its own main, a
malloc policy that fails the k-th allocation) built with the address and undefined-behaviour sanitizers and run as a child."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "buf_check.cpp")
BASE = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "krepp_amd", "csrc")]
SAN = ["-fsanitize=address,undefined"]  # (a report of either goes to stderr, which must stay empty)


def test_buf_check(tmp_path):
    exe = str(tmp_path / "buf_check")
    r = subprocess.run(BASE + SAN + [SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    sanitized = r.returncode == 0
    if not sanitized:  # no sanitizer runtime to link against: the same program without it (its own assertions still run)
        print("buf_check: built WITHOUT sanitizers:\n" + r.stdout)
        r = subprocess.run(BASE + [SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stdout, r.stderr, "(sanitized build)" if sanitized else "(plain build)")
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("buf_check: ok"), r.stdout
