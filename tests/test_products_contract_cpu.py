"""CPU: the refusals of the prediction-product entry points (ensemble, TTA views, calibration, smoothing, region votes,
label propagation, the pseudo-label monitor, kNN), held to a record of what the library answered BEFORE their launches
and alignment checks were moved onto csrc/rowgroup.hpp.  The companion of tests/test_api_contract_cpu.py.

tests/golden/products_contract.json was generated from the PARENT commit's library, not from this tree.  To regenerate
it, build the commit whose behaviour is the reference and run this module as a script with CMLPL_LIB naming that build:

    CMLPL_LIB=/path/to/reference/libcmlpl_hip.so python -m tests.test_products_contract_cpu

Every row is a malformed call with fake non-null pointers.  It is refused by the argument checks, which run in front of
any device call, so the pointers are never followed; a call that would pass them is never made (the recorder rejects a
row whose reference answer is not a negative CMLPL_E_* code).  A well-formed call gives every optional pointer, so each
pointer argument has its misaligned rows (by 1, 2, 4 or 8 bytes, below its type's alignment); a null optional pointer is
well-formed and therefore not a row.  Rows with two faults at once pin which check comes first."""
import ctypes as C
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "products_contract.json")
FAKE = 0x100000         # the first non-null "device pointer"; never dereferenced
BIG = 1 << 40
NAN, INF = float("nan"), float("inf")
N_, K_ = 8, 9           # rows and classes of the well-formed calls


def _betas(*v):
    return (C.c_float * len(v))(*v)


# An entry point's arguments in the header's order: "name" (a scalar), "name@A" (a device pointer that must be A-byte
# aligned), "name@A?" (the same, optional).  Pointers get distinct fake addresses 64 KiB apart: no two blocks overlap.
ENTRY = {
    "cmlpl_ensemble": ("logits@4 members member_stride weights n K labels@8 probs@4? conf@4? entropy@4? disagree@4? stream",
                       dict(members=2, member_stride=N_ * K_)),
    "cmlpl_ensemble_views": ("logits@4 members views member_stride view_stride weights n K labels@8 probs@4? conf@4? "
                             "entropy@4? disagree@4? stream",
                             dict(members=2, views=2, member_stride=2 * N_ * K_, view_stride=N_ * K_)),
    "cmlpl_reliability": ("probs@4 K row@8? truth@8 n bins counts@8 stream", dict(bins=15)),
    "cmlpl_temper_probs": ("probs@4 n K beta out@4? labels@8? conf@4? entropy@4? stream", dict(beta=0.5)),
    "cmlpl_nll_temps": ("probs@4 K row@8? truth@8 n betas S sums@8 stream", dict(betas=_betas(0.5, 1.0, 2.0), S=3)),
    "cmlpl_smooth_probs": ("probs@4 guide@4 guide_stride guide_ch rows cols K radius sigma_s sigma_r out@4? labels@8? conf@4? "
                           "entropy@4? stream",
                           dict(guide_stride=16, guide_ch=3, rows=2, cols=4, radius=2, sigma_s=2.0, sigma_r=0.5)),
    "cmlpl_sp_vote_probs": ("seg@4 probs@4 n K N out_probs@4? labels@8? conf@4? entropy@4? sums@8? cnt@8? seg_probs@4? "
                            "seg_labels@8? ws@8 ws_bytes stream", dict(N=4, ws_bytes=BIG)),
    "cmlpl_sp_vote_labels": ("seg@4 src@8 n K N out_probs@4? labels@8? conf@4? entropy@4? sums@8? cnt@8? seg_probs@4? "
                             "seg_labels@8? ws@8 ws_bytes stream", dict(N=4, ws_bytes=BIG)),
    "cmlpl_lp_graph": ("idx@4 sim@4 n k gamma graph@4 bytes stream", dict(k=4, gamma=3, bytes=BIG)),
    "cmlpl_lp_propagate": ("graph@4 n k Y@4 K alpha iters F0@4? F@4 tmp@4 probs@4? labels@8? conf@4? entropy@4? residual@4? "
                           "stream", dict(k=4, alpha=0.9, iters=3)),
    "cmlpl_pl_stats": ("probs@4 n K truth@8 idx@8? adap pos neg counts@8 stream", dict(adap=0.5, pos=0.8, neg=0.3)),
    "cmlpl_pl_stats_hard": ("pseudo@8 n K truth@8 idx@8? counts@8 stream", {}),
    "cmlpl_knn": ("query@16 n gallery@16 m labels_g@8 K skip@8? k inv_T nbr_idx@4? nbr_sim@4? probs@4? labels@8? ws@16 "
                  "ws_bytes stream", dict(m=N_, k=4, inv_T=1.0, ws_bytes=BIG)),
}


def _spec(fn):
    """[(name, alignment or 0, optional)] of fn's arguments, and the values of a well-formed call"""
    order, over = ENTRY[fn]
    args, vals = [], dict(n=N_, K=K_, stream=None, weights=None)
    for i, word in enumerate(order.split()):
        name, _, al = word.partition("@")
        args.append((name, int(al.rstrip("?") or 0), al.endswith("?")))
        if al:
            vals[name] = FAKE + (i << 16)
    vals.update(over)
    return args, vals


def call(lib, fn, over):
    args, vals = _spec(fn)
    vals.update(over)
    return getattr(lib, fn)(*[vals[name] for name, _, _ in args])


def _rows():
    rows = []

    def add(fn, tag, **over):
        rows.append((f"{fn[6:]}:{tag}", fn, over))

    for fn in ENTRY:
        args, vals = _spec(fn)
        ptrs = [(name, al, opt) for name, al, opt in args if al]
        for name, al, opt in ptrs:
            for off in (1, 2, 4, 8):
                if off < al:
                    add(fn, f"{name}+{off}", **{name: vals[name] + off})
            if not opt:
                add(fn, f"null-{name}", **{name: None})
        first, last = ptrs[0][0], ptrs[-1][0]
        for tag, o in (("K-0", dict(K=0)), ("K-65", dict(K=65)), ("n-0", dict(n=0)), ("n-neg", dict(n=-1))):
            if fn == "cmlpl_lp_graph" and tag[0] == "K":
                continue
            if fn == "cmlpl_smooth_probs" and tag[0] == "n":
                o = dict(rows=o["n"])
            add(fn, tag, **o)
            add(fn, f"{tag}+{last}+1", **o, **{last: vals[last] + 1})           # two faults: the counts come first
        add(fn, f"{first}+1+{last}+2", **{first: vals[first] + 1, last: vals[last] + 2})

    for fn in ("cmlpl_ensemble", "cmlpl_ensemble_views"):
        add(fn, "members-0", members=0)
        add(fn, "member-stride-short", member_stride=N_ * K_ - 1)
        add(fn, "weights-negative", weights=_betas(1.0, -1.0)); add(fn, "weights-nan", weights=_betas(1.0, NAN))
        add(fn, "weights-inf", weights=_betas(1.0, INF)); add(fn, "weights-zero", weights=_betas(0.0, 0.0))
        add(fn, "weights-negative+probs+2", weights=_betas(1.0, -1.0), probs=_spec(fn)[1]["probs"] + 2)   # alignment first
        add(fn, "stride-short+labels+4", member_stride=1, labels=_spec(fn)[1]["labels"] + 4)
    add("cmlpl_ensemble", "members-5", members=5, member_stride=N_ * K_)
    fn = "cmlpl_ensemble_views"
    add(fn, "views-0", views=0); add(fn, "members-65", members=65, views=1); add(fn, "views-65", members=1, views=65)
    add(fn, "blocks-66", members=2, views=33, member_stride=33 * N_ * K_)
    add(fn, "view-stride-short", view_stride=N_ * K_ - 1)
    add(fn, "views-overlap-members", member_stride=2 * N_ * K_ - 1)
    fn = "cmlpl_reliability"
    add(fn, "bins-0", bins=0); add(fn, "bins-1025", bins=1025); add(fn, "bins-0+counts+4", bins=0, counts=FAKE + 4)
    fn = "cmlpl_temper_probs"
    for tag, b in (("beta-0", 0.0), ("beta-neg", -1.0), ("beta-nan", NAN), ("beta-inf", INF)):
        add(fn, tag, beta=b)
        add(fn, tag + "+out+2", beta=b, out=_spec(fn)[1]["out"] + 2)
    fn = "cmlpl_nll_temps"
    add(fn, "S-0", S=0); add(fn, "S-65", S=65); add(fn, "null-betas", betas=None)
    add(fn, "beta-small", betas=_betas(0.5, 0.01, 2.0)); add(fn, "beta-large", betas=_betas(0.5, 1.0, 17.0))
    add(fn, "beta-nan", betas=_betas(NAN, 1.0, 2.0)); add(fn, "beta-inf", betas=_betas(0.5, 1.0, INF))
    add(fn, "beta-nan+sums+4", betas=_betas(NAN, 1.0, 2.0), sums=_spec(fn)[1]["sums"] + 4)
    fn = "cmlpl_smooth_probs"
    v = _spec(fn)[1]
    add(fn, "radius-0", radius=0); add(fn, "radius-65", radius=65); add(fn, "cols-0", cols=0)
    add(fn, "guide_ch-neg", guide_ch=-1); add(fn, "guide_ch-65", guide_ch=65, guide_stride=65)
    add(fn, "guide-null", guide=None); add(fn, "guide-stride-short", guide_stride=2)
    add(fn, "scene-too-large", rows=1 << 16, cols=1 << 16)
    for tag, o in (("sigma_s-0", dict(sigma_s=0.0)), ("sigma_s-nan", dict(sigma_s=NAN)), ("sigma_s-inf", dict(sigma_s=INF)),
                   ("sigma_r-0", dict(sigma_r=0.0)), ("sigma_r-nan", dict(sigma_r=NAN)), ("sigma_r-neg", dict(sigma_r=-1.0)),
                   ("sigma_s-tiny", dict(sigma_s=1e-30))):
        add(fn, tag, **o)
    add(fn, "no-output", out=None, labels=None)
    add(fn, "in-place", out=v["probs"]); add(fn, "overlap", out=v["probs"] + 4 * K_)
    add(fn, "sigma_s-0+conf+1", sigma_s=0.0, conf=v["conf"] + 1); add(fn, "in-place+labels+4", out=v["probs"], labels=v["labels"] + 4)
    add(fn, "sigma_s-tiny+entropy+2", sigma_s=1e-30, entropy=v["entropy"] + 2)
    for fn in ("cmlpl_sp_vote_probs", "cmlpl_sp_vote_labels"):
        v = _spec(fn)[1]
        add(fn, "N-0", N=0); add(fn, "table-too-large", N=1 << 26, K=64); add(fn, "ws-short", ws_bytes=12 * 4 * (K_ + 2) - 1)
        add(fn, "ws-0", ws_bytes=0)
        add(fn, "no-output", **{k: None for k in "out_probs labels conf entropy sums cnt seg_probs seg_labels".split()})
        add(fn, "ws-short+seg+2", ws_bytes=0, seg=v["seg"] + 2); add(fn, "N-0+ws-short", N=0, ws_bytes=0)
    fn = "cmlpl_lp_graph"
    v = _spec(fn)[1]
    add(fn, "k-0", k=0); add(fn, "k-33", k=33); add(fn, "gamma-0", gamma=0); add(fn, "gamma-9", gamma=9)
    add(fn, "entries-2^31", n=1 << 27, k=16)
    add(fn, "bytes-short", bytes=64); add(fn, "bytes-0", bytes=0)
    for nm in ("idx", "sim", "graph"):                                           # CMLPL_E_ARG before CMLPL_E_WORKSPACE
        add(fn, f"{nm}+2+bytes-short", **{nm: v[nm] + 2}, bytes=64)
    add(fn, "gamma-0+bytes-short", gamma=0, bytes=0); add(fn, "null-graph+bytes-short", graph=None, bytes=0)
    fn = "cmlpl_lp_propagate"
    v = _spec(fn)[1]
    for tag, a in (("alpha-1", 1.0), ("alpha-neg", -0.25), ("alpha-nan", NAN), ("alpha-inf", INF)):
        add(fn, tag, alpha=a)
    add(fn, "iters-0", iters=0); add(fn, "iters-10001", iters=10001); add(fn, "k-0", k=0); add(fn, "k-33", k=33)
    add(fn, "rows-2^31", n=1 << 26, k=1, K=32)
    add(fn, "F-is-tmp", tmp=v["F"]); add(fn, "F0-is-F", F0=v["F"]); add(fn, "F0-is-tmp", F0=v["tmp"])
    add(fn, "Y-is-F", Y=v["F"]); add(fn, "Y-is-tmp", Y=v["tmp"]); add(fn, "start-Y-is-F", F0=None, F=v["Y"])
    add(fn, "alpha-1+probs+2", alpha=1.0, probs=v["probs"] + 2); add(fn, "F-is-tmp+labels+4", tmp=v["F"], labels=v["labels"] + 4)
    add(fn, "iters-0+residual+1", iters=0, residual=v["residual"] + 1)
    fn = "cmlpl_knn"
    v = _spec(fn)[1]
    add(fn, "m-0", m=0); add(fn, "k-0", k=0); add(fn, "k-33", k=33)
    add(fn, "inv_T-0", inv_T=0.0); add(fn, "inv_T-nan", inv_T=NAN); add(fn, "inv_T-inf", inv_T=INF)
    search = dict(labels_g=None, K=0, probs=None, labels=None)
    add(fn, "search-with-K", **dict(search, K=K_)); add(fn, "search-with-probs", **dict(search, probs=v["probs"]))
    add(fn, "search-with-labels", **dict(search, labels=v["labels"]))
    add(fn, "ws-short", ws_bytes=1024); add(fn, "ws-0", ws_bytes=0); add(fn, "search-ws-short", **search, ws_bytes=1024)
    for nm, off in (("query", 8), ("skip", 4), ("nbr_sim", 2)):                  # CMLPL_E_ARG before CMLPL_E_WORKSPACE
        add(fn, f"{nm}+{off}+ws-short", **{nm: v[nm] + off}, ws_bytes=1024)
    add(fn, "inv_T-0+ws-short", inv_T=0.0, ws_bytes=0)
    assert len({r[0] for r in rows}) == len(rows)
    return rows


ROWS = _rows()


def collect(lib):
    """everything the fixture holds, from `lib`"""
    refusals = {}
    for rid, fn, over in ROWS:
        rc = call(lib, fn, over)
        if not -3 <= rc <= -1:
            raise AssertionError(f"{rid}: the reference answers {rc}: not a refusal, the row does not belong in the table")
        refusals[rid] = rc
    return {"refusals": refusals}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from cmlpl_amd import _lib
    return _lib.load()


def test_the_table_is_the_recorded_one(golden):
    assert sorted(golden["refusals"]) == sorted(r[0] for r in ROWS)
    assert all(-3 <= rc <= -1 for rc in golden["refusals"].values())
    by_fn = {fn: [golden["refusals"][r[0]] for r in ROWS if r[1] == fn] for fn in ENTRY}
    assert all(by_fn.values())                                   # every entry point has rows
    assert -3 in by_fn["cmlpl_lp_graph"] and -3 in by_fn["cmlpl_knn"]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_refusal_is_the_parents(row, lib, golden):
    rid, fn, over = row
    assert call(lib, fn, over) == golden["refusals"][rid]


if __name__ == "__main__":
    from cmlpl_amd import _lib
    if not os.environ.get("CMLPL_LIB"):
        raise SystemExit("name the reference build with CMLPL_LIB: the record is not taken from the tree under test")
    record = collect(_lib.load())
    with open(FIXTURE, "w") as f:
        json.dump(record, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(ROWS), "refusals")
