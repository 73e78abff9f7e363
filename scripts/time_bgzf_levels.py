#!/usr/bin/env python3
"""Device time of the BGZF deflate kernels at level 1 and level 2 on ~110 MB of report-shaped text (docs/design/15 section 15.6).

usage: scripts/time_bgzf_levels.py [rounds, default 3]
       scripts/time_bgzf_levels.py --arm ROOT LEVEL     (one arm, in a process of its own: what the first form starts)

The text is tests/deflate_cases.report_text(5000) twenty times over (members are coded on their own and the period is far beyond
the 32 KB a match may reach back, so the ratio is the fixture's).  Every arm is a fresh process that uploads the toy index, opens a
stream and sends the text through kr_debug_bgzf_deflate four times; kr_debug_bgzf_deflate_ms gives the deflate, scan and copy
kernels of repetitions 1 .. 3.  Arms alternate within a round: the tree KR_TIME_BGZF_PARENT_ROOT names (another commit, built, as
the yardstick of the same session; its encoder has no levels), this tree at level 1, this tree at level 2."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arm(root, level):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import deflate_cases as dc
    from krepp_amd import capi

    text = dc.report_text(5000) * 20
    hx = capi.HostIndex(os.path.join(HERE, "tests", "golden", "toy_index"))
    dx = hx.upload(0)
    st = dx.stream(max_reads=64, max_bases=1 << 16)
    st.text_enable(hx, 1 << 16, 1 << 12)
    st.bgzf_out_enable()
    if level:
        st.bgzf_out_level(level)
    st.bgzf_deflate_ms()  # (makes the events)
    ms, size = [], 0
    for _ in range(4):
        size = len(st.bgzf_deflate(text))
        ms.append(st.bgzf_deflate_ms())
    st.close(), dx.close(), hx.close()
    best = min(ms[1:])
    print("%-28s level %s: %d bytes of text -> %d (%.4f); kernels %s ms; best %.2f ms = %.1f GB/s of text"
          % (os.path.relpath(root, HERE) if root != HERE else "this tree", level or "-", len(text), size, size / len(text),
             " ".join("%.2f" % m for m in ms[1:]), best, len(text) / best / 1e6), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--arm":
        arm(sys.argv[2], int(sys.argv[3]))
        sys.exit(0)
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    parent = os.environ.get("KR_TIME_BGZF_PARENT_ROOT")
    arms = ([(parent, 0)] if parent else []) + [(HERE, 1), (HERE, 2)]
    for r in range(rounds):
        print("round %d" % (r + 1), flush=True)
        for root, level in arms:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", root, str(level)], timeout=300).returncode
            if rc:  # nothing more is started on the device behind a failed arm
                sys.exit("arm %s level %d ended with status %d" % (root, level, rc))
