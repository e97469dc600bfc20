"""What the launches of tests/ssd_wave_cases.py contain, from their geometry alone (numpy, no GPU): every situation
that tests/test_ssd_wave_gpu.py is meant to put before ssd_disparity_kernel must really be in the list. A list that
lost its border keypoints, its 65-column maps or its tracker offsets fails here."""
import collections

import numpy as np

import ssd_wave_cases as SW
import window_cases as WC


def _launch_geometry():
    """per launch and sequence: the geometry of the keypoints the launch handles"""
    geo = {}
    for launch in SW.launches():
        for b, s in enumerate(launch["seqs"]):
            name = s["case"][0]
            if name not in geo:
                geo[name] = SW.geometry(s["case"])
            g = geo[name]
            lo = s["first"] + (s["first_dev"] or 0)
            hi = min(len(s["idx"]), lo + launch["n_bound"])
            handled = s["idx"][lo:hi] if s["enable"] != 0 and hi > lo else s["idx"][:0]
            yield launch, b, s, {k: v[handled] for k, v in g.items()}


def test_every_case_of_the_window_list_is_launched():
    names = {l["seqs"][0]["case"][0] for l in SW.launches() if l["name"].startswith("case-")}
    assert names >= {c[0] for c in WC.ssd_cases()} and names >= {c[0] for c in SW.extra_cases()}
    for l in SW.launches():
        if l["name"].startswith("case-"):
            s = l["seqs"][0]
            assert len(s["idx"]) == len(s["case"][3]) == l["n_bound"] and s["first"] == 0 and not s["first_dev"] and s["enable"] is None
    for c in SW.extra_cases():
        assert c[1].shape in ((SW.SMALL_H, SW.SMALL_W), (SW.BIG_H, SW.BIG_W)) and c[1].shape == c[2].shape


def test_launches_reach_what_they_claim():
    seen = collections.defaultdict(set)          # per kernel shape (31 / 35)
    short = collections.defaultdict(set)
    skips = collections.defaultdict(lambda: collections.Counter())
    edges = collections.defaultdict(lambda: collections.Counter())
    counts = collections.defaultdict(set)
    forms = collections.Counter()
    batches = collections.defaultdict(set)
    for launch, b, s, g in _launch_geometry():
        case = s["case"]
        shape = SW.shape_of(launch["win"], launch["search_y"])
        win, sx, sy, clamp = case[4:]
        assert win <= launch["win"] and sy <= launch["search_y"] and sx <= 64
        ok = ~g["skipped"]
        seen[shape] |= {("win", win, sy)}
        seen[shape] |= {("mw", int(v)) for v in g["mw"][ok]} | {("col_blocks", int(v + 15) // 16) for v in g["mw"][ok]}
        seen[shape] |= {("row_blocks", int(v + 15) // 16) for v in g["mh"][ok]}
        # which of the four sizes fall short of what the settings give in the image's middle
        wa_wb = win // 2 + (win + 1) // 2
        full = dict(tw=wa_wb, th=wa_wb, mw=sx + 1, mh=2 * sy + 1)
        for f, v in full.items():
            if (g[f][ok] < v).any():
                short[shape].add(f)
        if name_is_random_bytes(case[0]):
            for f, v in full.items():
                if (g[f][ok] < v).any():
                    short[shape, "random"].add(f)
        skips[shape][clamp] += int(g["skipped"].sum())
        off, stride = SW.LAYOUTS[s["layout"]][0], SW.LAYOUTS[s["layout"]][1](case[1].shape[1])
        if ok.any():
            edges[shape]["stride != width"] += stride != case[1].shape[1]
            edges[shape][f"base off {off}"] += 1
            edges[shape]["edge16"] += int(g["edge16"][ok].sum())
            edges[shape]["edge4"] += int(g["edge4"][ok].sum())
        if launch["name"].startswith("count"):
            counts[shape].add(len(s["idx"]))
        if launch["name"].startswith("tracker"):
            batches[shape].add(len(launch["seqs"]))
            n = len(s["idx"])
            lo = s["first"] + (s["first_dev"] or 0)
            forms[shape, "first > 0"] += s["first"] > 0
            forms[shape, "*first_ptr > 0"] += bool(s["first_dev"])
            forms[shape, "no first_ptr"] += s["first_dev"] is None
            forms[shape, "n_bound beyond n"] += lo + launch["n_bound"] > n and lo < n
            forms[shape, "n_bound short of n"] += lo + launch["n_bound"] < n
            forms[shape, "enable 0"] += s["enable"] == 0
            forms[shape, "enable not 0 and not 1"] += s["enable"] not in (None, 0, 1)
            forms[shape, "no enable"] += s["enable"] is None
            forms[shape, "other settings than the launch's"] += (win, sy) != (launch["win"], launch["search_y"])
    for shape in (31, 35):
        print(shape, sorted(short[shape]), dict(skips[shape]), dict(edges[shape]), sorted(counts[shape]), sorted(batches[shape]),
              {k[1]: v for k, v in forms.items() if k[0] == shape})
        assert short[shape] == {"tw", "th", "mw", "mh"} and short[shape, "random"] == {"tw", "th", "mw", "mh"}
        assert skips[shape][0] > 0 and skips[shape][1] > 0, "keypoints skipped with and without clamp_half"
        assert {e[1] for e in seen[shape] if e[0] == "col_blocks"} == {1, 2, 3, 4, 5}
        assert ("mw", 65) in seen[shape] and ("mw", 1) in seen[shape]
        for want in ("stride != width", "base off 1", "base off 2", "base off 3", "edge16", "edge4"):
            assert edges[shape][want] > 0, want
        assert counts[shape] == set(SW.COUNTS)
        assert batches[shape] == set(SW.BATCHES)
        for k in ("first > 0", "*first_ptr > 0", "no first_ptr", "n_bound beyond n", "n_bound short of n", "enable 0",
                  "enable not 0 and not 1", "no enable", "other settings than the launch's"):
            assert forms[shape, k] > 0, (shape, k)
    assert {e[1:] for e in seen[31] if e[0] == "win"} >= {(31, 6)}
    assert {e[1:] for e in seen[35] if e[0] == "win"} >= {(33, 7), (35, 8)}
    assert {e[1] for e in seen[31] if e[0] == "row_blocks"} == {1}
    assert {e[1] for e in seen[35] if e[0] == "row_blocks"} == {1, 2}


def name_is_random_bytes(name):
    return name.startswith(("border-", "big-", "blocks-w"))


def test_border_points_lie_where_they_should():
    """0 .. 4 px from every border and corner, and the clamp_half rule decides some of the points outside"""
    for h, w in ((SW.SMALL_H, SW.SMALL_W), (SW.BIG_H, SW.BIG_W)):
        p = SW.border_points(h, w).astype(np.int64)
        for d in range(5):
            for x in (d, w - 1 - d):
                for y in (d, h - 1 - d):
                    assert ((p[:, 0] == x) & (p[:, 1] == y)).any(), (x, y)           # the corners
            assert ((p[:, 0] == d) & (p[:, 1] == 30)).any() and ((p[:, 0] == w - 1 - d) & (p[:, 1] == 30)).any()
            assert ((p[:, 1] == d) & (p[:, 0] == 40)).any() and ((p[:, 1] == h - 1 - d) & (p[:, 0] == 40)).any()
    for win, sy in SW.SHAPES:
        g1 = SW.geometry(SW.case_by_name(f"border-w{win}-sy{sy}-c1"))
        g0 = SW.geometry(SW.case_by_name(f"border-w{win}-sy{sy}-c0"))
        assert (g1["skipped"] & ~g0["skipped"]).any() and (g1["skipped"] & g0["skipped"]).any() and (~g1["skipped"]).sum() > 100


def test_expected_words():
    s = dict(idx=np.arange(10), first=1, first_dev=2, enable=None)
    d = np.arange(10, dtype=np.float32)
    e = SW.expected(s, d, 4, 14)
    assert (e[3:7].view(np.float32) == d[3:7]).all() and (np.delete(e, range(3, 7)) == SW.FILL).all()
    assert (SW.expected(dict(s, enable=0), d, 4, 14) == SW.FILL).all()
    e = SW.expected(dict(s, enable=0x100, first_dev=None), d, 50, 14)
    assert (e[1:10].view(np.float32) == d[1:]).all() and e[0] == SW.FILL and (e[10:] == SW.FILL).all()
