"""tests/select_ref.py held to the oracle (no GPU): the toy index, the toy reads and 200 reverse-complement palindromes, in six report
modes.  Both strands of a palindrome give the same histogram, hence equal d and equal match counts: the inputs that make the strand
merge's tie rule and the closest's (strand, index) order matter.  The restatement is fed the oracle's accumulators that passed the
hdist_filt test and must print the oracle's rows."""
import numpy as np
import pytest

from helpers import revcomp
from select_ref import select_ref

MODES = [dict(), dict(multi=0), dict(dist_max=0.05), dict(multi=0, dist_max=0.05), dict(no_filter=0), dict(no_filter=0, dist_max=0.08)]


@pytest.fixture(scope="module")
def batch(toy_reads):
    names, bases, offs = toy_reads
    seqs = [bytes(bases[int(offs[i]):int(offs[i + 1])]).decode() for i in range(len(names))]
    pal = [s[:75] + revcomp(s[:75]) for s in seqs if len(s) >= 75 and set(s[:75]) <= set("ACGT")][:200]
    assert len(pal) == 200
    allseq = seqs + pal
    b = np.frombuffer("".join(allseq).encode(), np.uint8)
    o = np.cumsum([0] + [len(s) for s in allseq]).astype(np.uint64)
    return b, o, list(names) + [f"pal{i}" for i in range(len(pal))]


@pytest.mark.parametrize("mode", MODES, ids=lambda m: ",".join(f"{k}={v}" for k, v in m.items()) or "default")
def test_select_ref_prints_the_oracles_rows(po, toy_index_dir, batch, mode):
    bases, offs, names = batch
    ix = po.Index(toy_index_dir)
    p = po.params(collect=1, **mode)
    ref = ix.dist(bases, offs, names, p)
    k, h, th = ix.info.k, ix.info.h, p.hdist_th
    accs = ref["accs"][ref["accs"]["passed"] != 0]
    order = np.lexsort((accs["strand"], accs["se"], accs["read"]))  # read, then key = se << 1 | strand
    accs = accs[order]
    bounds = np.searchsorted(accs["read"], np.arange(len(names) + 1))
    got, pair_ties, closest_ties = [], 0, 0
    for r in range(len(names)):
        a = accs[bounds[r]:bounds[r + 1]]
        recs = [((int(x["se"]) << 1) | int(x["strand"]), float(x["d_llh"]), float(x["v_llh"]), int(x["match_count"])) for x in a]
        onmers = int(ref["reads"]["onmers"][r])

        def f(ic, d, a=a, onmers=onmers):
            return po.llh(k, h, th, a[ic]["hist"][:th + 1].astype(np.float64), float(onmers - int(a[ic]["match_count"])), float(a[ic]["rho"]), d)

        out = select_ref(recs, multi=p.multi, no_filter=p.no_filter, dist_max=p.dist_max, chisq=p.chisq, f=f)
        got += [(r, key >> 1, key & 1) for key, _d in out["rows"]]
        pair_ties += sum(1 for x, y in zip(recs, recs[1:]) if x[0] ^ 1 == y[0] and x[1] == y[1])
        ds = sorted(x[1] for x in recs)
        closest_ties += len(ds) >= 2 and ds[0] == ds[1]
    rows = ref["rows"][ref["rows"]["se"] != 0]  # (se 0: the NA row of a read)
    want = [(int(x["read"]), int(x["se"]), int(x["strand"])) for x in rows]
    print(f"rows {len(want)}, strand pairs with equal d {pair_ties}, reads whose two smallest d are equal {closest_ties}")
    assert pair_ties > 0 and closest_ties > 0  # the anchor keeps its point
    assert sorted(got) == sorted(want)
    assert got == want  # ... and in the oracle's order: read by read, ascending se
