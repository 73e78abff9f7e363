"""An independent numpy restatement of `krepp inspect` (Index::display_info, FlatHT::display_info, CRecord::display_info of the
reference), from the index FILES: the expected statistics and the expected text of tests/test_inspect_cpu.py and of the GPU tests.
Nothing here calls the library under test, except craft_view, which only lays numpy arrays out as a kr_index_view."""
import ctypes as C
import os
import re
import struct

import numpy as np


# ---- statistics -------------------------------------------------------------------------------------------------------------
def stats_ref(se, pse, nsubsets):
    """se: the colour column of cmer; pse: [nsubsets, 2].  All ids must be < nsubsets (np.bincount would grow silently)."""
    se = np.asarray(se, dtype=np.int64)
    pse = np.asarray(pse, dtype=np.int64).reshape(-1, 2)
    assert len(pse) == nsubsets and (se < nsubsets).all() and (pse[1:] < nsubsets).all()
    count = np.bincount(se, minlength=nsubsets).astype(np.uint64)
    outdeg = (np.bincount(pse[1:, 0], minlength=nsubsets) + np.bincount(pse[1:, 1], minlength=nsubsets)).astype(np.uint64)
    mv, mf = np.unique(count[1:], return_counts=True)
    dv, df = np.unique(outdeg[1:], return_counts=True)
    return {"nkmers": len(se), "nsubsets": nsubsets, "se_count": count, "se_outdeg": outdeg, "mer_value": mv.astype(np.uint64),
            "mer_freq": mf.astype(np.uint64), "deg_value": dv.astype(np.uint64), "deg_freq": df.astype(np.uint64)}


def assert_stats_equal(got, want, counts=True):
    for k in ("nkmers", "nsubsets"):
        assert got[k] == want[k], k
    for k in ("mer_value", "mer_freq", "deg_value", "deg_freq") + (("se_count", "se_outdeg") if counts else ()):
        assert got[k] is not None, k
        np.testing.assert_array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64), err_msg=k)
    if not counts:
        assert got["se_count"] is None and got["se_outdeg"] is None
    if want["nsubsets"] >= 1:
        assert int(np.asarray(got["mer_freq"], np.uint64).sum()) == want["nsubsets"] - 1
        assert int(np.asarray(got["deg_freq"], np.uint64).sum()) == want["nsubsets"] - 1


# ---- index files ------------------------------------------------------------------------------------------------------------
def suffixes(index_dir):
    return sorted(f[len("metadata"):] for f in os.listdir(index_dir) if f.startswith("metadata-") and "." not in f)


def read_lib(index_dir, sfx):
    md = open(os.path.join(index_dir, "metadata" + sfx), "rb").read()
    k, w, h, m, r, frac, nrows = struct.unpack_from("<BBBIIBI", md, 0)
    pos = np.frombuffer(md, np.uint8, k, 16)
    cm = open(os.path.join(index_dir, "cmer" + sfx), "rb").read()
    nk = struct.unpack_from("<Q", cm, 0)[0]
    cmer = np.frombuffer(cm, np.uint32, 2 * nk, 8).reshape(-1, 2)
    cr = open(os.path.join(index_dir, "crecord" + sfx), "rb").read()
    nnodes, nsubsets = struct.unpack_from("<II", cr, 0)
    pse = np.frombuffer(cr, np.uint32, 2 * nsubsets, 8).reshape(-1, 2)
    return dict(k=k, w=w, h=h, m=m, r=r, frac=frac, ppos=pos[:h], npos=pos[h:], nkmers=nk, cmer=cmer, nsubsets=nsubsets, pse=pse, nnodes=nnodes)


def info_text(index_dir, sfx, L):
    p = os.path.join(index_dir, "metadata" + sfx + ".txt")
    if os.path.exists(p):
        return open(p, "rb").read().decode()
    lst = lambda v: "[" + ", ".join(str(int(x)) for x in v) + "]"
    return ("krepp version: ?\ndate: ?\nseed: ?\n" + "k: %d\nw: %d\nh: %d\nm: %d\n" % (L["k"], L["w"], L["h"], L["m"]) +
            "frac: %s\n" % ("true" if L["frac"] else "false") + "ppos_v: %s\nnpos_v: %s\n" % (lst(L["ppos"]), lst(L["npos"])) +
            "nrows: %d\ntotal_num_kmers: %d\nsdust-t: ?\nsdust-w: ?\n" % (4 ** L["h"], L["nkmers"]))


def newick_basic(text):
    """The tree file re-emitted as Tree::stream_nwk_basic does: labels as written, branch lengths in %g form, nothing else.
    (Plain Newick only: no quotes or comments, as in the trees of the tests.)"""
    toks = re.findall(r"[(),;]|[^(),;]+", text.strip())
    out = []
    for t in toks:
        if t in "(),;":
            out.append(t)
            continue
        label, _, blen = t.partition(":")
        out.append(label.strip())
        if blen.strip():
            out.append(":%g" % float(blen))
    s = "".join(out)
    return s if s.endswith(";") else s + ";"


def inspect_text(index_dir):
    sfxs = suffixes(index_dir)
    tree = os.path.join(index_dir, "tree" + sfxs[0])
    out = "Backbone tree: " + (newick_basic(open(tree).read()) if os.path.exists(tree) else "NA") + "\n"
    by_key = {}
    for sfx in sfxs:
        L = read_lib(index_dir, sfx)
        S = stats_ref(L["cmer"][:, 1], L["pse"], L["nsubsets"])
        for key in (range(L["r"] + 1) if L["frac"] else [L["r"]]):
            by_key[key] = (sfx, L, S)
    for key in sorted(by_key):
        sfx, L, S = by_key[key]
        out += "======= Partial index: %d =======\n" % key + info_text(index_dir, sfx, L)
        out += "%d\tNUM_COLORS\t%d\n" % (key, L["nsubsets"] - 1)
        out += "".join("%d\tMER_COUNT\t%d\t%d\n" % (key, v, f) for v, f in zip(S["mer_value"], S["mer_freq"]))
        out += "".join("%d\tOUTDEGREE_COUNT\t%d\t%d\n" % (key, v, f) for v, f in zip(S["deg_value"], S["deg_freq"]))
    return out.encode()


def write_index(index_dir, libs, names, k=21, h=7, m=4, nwk=None):
    """A tiny index directory in the on-disk layout: libs = dicts(r, frac, se, pse[, info]); the tree is the balanced tree over
    `names` (2 * len(names) - 1 nodes) unless `nwk` is given (its node count must match)."""
    os.makedirs(index_dir, exist_ok=True)
    ppos = np.arange(k - 1, k - 1 - h, -1, dtype=np.uint8)
    npos = np.arange(0, k - h, dtype=np.uint8)
    nnodes = 2 * len(names)  # crecord's nnodes = tree nodes + 1
    for L in libs:
        sfx = "-m%dr%d-%s" % (m, L["r"], "frac" if L["frac"] else "no_frac")
        se = np.asarray(L["se"], np.uint32)
        pse = np.asarray(L["pse"], np.uint32).reshape(-1, 2)
        cmer = np.stack([np.arange(len(se), dtype=np.uint32), se], axis=1) if len(se) else np.zeros((0, 2), np.uint32)
        with open(os.path.join(index_dir, "metadata" + sfx), "wb") as f:
            f.write(struct.pack("<BBBIIBI", k, k + 6, h, m, L["r"], 1 if L["frac"] else 0, 4) + ppos.tobytes() + npos.tobytes())
        with open(os.path.join(index_dir, "cmer" + sfx), "wb") as f:
            f.write(struct.pack("<Q", len(se)) + cmer.tobytes())
        with open(os.path.join(index_dir, "inc" + sfx), "wb") as f:
            f.write(struct.pack("<I", 4) + np.full(4, len(se), np.uint64).tobytes())
        with open(os.path.join(index_dir, "crecord" + sfx), "wb") as f:
            f.write(struct.pack("<II", nnodes, len(pse)) + pse.tobytes() + np.zeros(nnodes, np.float64).tobytes())
        with open(os.path.join(index_dir, "reflist" + sfx), "w") as f:
            f.write("".join(n + "\n" for n in names))
        if nwk is not None:
            with open(os.path.join(index_dir, "tree" + sfx), "w") as f:
                f.write(nwk)
        if "info" in L:
            with open(os.path.join(index_dir, "metadata" + sfx + ".txt"), "w") as f:
                f.write(L["info"])
    return index_dir


# ---- crafted views ----------------------------------------------------------------------------------------------------------
def craft_view(capi, libs, m=4):
    """A kr_index_view over numpy arrays: libs = dicts(se, pse[, r, frac]) or (cmer_ptr, pse_ptr, nkmers, nsubsets) as 'ptrs' for
    arrays that are elsewhere (device memory).  Returns (view, keep): hold on to `keep` while the view is in use."""
    arr = (capi.KrLibView * len(libs))()
    keep = [arr]
    for i, L in enumerate(libs):
        if "ptrs" in L:
            cp, pp, nk, ns = L["ptrs"]
        else:
            se = np.asarray(L["se"], np.uint32)
            cmer = np.ascontiguousarray(np.stack([np.arange(len(se), dtype=np.uint32) * np.uint32(2654435761), se], axis=1)) if len(se) else np.zeros((1, 2), np.uint32)
            pse = np.ascontiguousarray(np.asarray(L["pse"], np.uint32).reshape(-1, 2))
            keep += [cmer, pse]
            cp, pp, nk, ns = cmer.ctypes.data, pse.ctypes.data, len(se), len(pse)
        arr[i].cmer = C.cast(cp, capi.u32p)
        arr[i].pse = C.cast(pp, capi.u32p)
        arr[i].nkmers, arr[i].nsubsets, arr[i].nnodes = nk, ns, 2
        arr[i].r, arr[i].frac = L.get("r", 1), L.get("frac", 1)
    view = capi.KrIndexView(k=21, h=7, m=m, nlibs=len(libs), tree_nnodes=1)
    view.libs = arr
    return view, keep
