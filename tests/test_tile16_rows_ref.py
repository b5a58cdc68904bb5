"""The block-row plan of the 16x16 search without a device (tests/tile16_rows_ref.py): numbers worked out by hand, the
census of the device cases, the byte extents as a property over every width, both origins and every predictor, and the
model's grid and skipped columns held to aof.grid and to the oracle's records."""
import numpy as np
import pytest

import batch_plan_ref as plan_ref
import tile16_rig as rig
import tile16_rows_ref as ref

_refs = {}


def oracle_of(aof, orc, synth, c, k=0, gate_off=False):
    """(params, prevs, curs, names, oracle records) of batch k of a case, computed once."""
    key = (c["id"], k, gate_off)
    if key not in _refs:
        p = rig.case_params(aof, c)
        assert aof.check_params(p) == 0, c["id"]
        prevs, curs, names = rig.case_frames(c, synth, ref, k)
        po = orc.params_from(p)
        if gate_off:
            po.feature_threshold = 0
        _refs[key] = (p, prevs, curs, names, [orc.flow_pair(po, prevs[i], curs[i], want_l1=True) for i in range(prevs.shape[0])])
    return _refs[key]


def case_preds(aof, orc, synth, c, k=0):
    return rig.preds_of(oracle_of(aof, orc, synth, c, k)[4]) if c["levels"] == 2 else None


def wg(w, h, org=0, by=0, px=0, py=0, pair=0, n=1, prune=0, refine=False, hint=0):
    nx, ny = ref.grid(w, h, org)
    return ref.workgroup(w, h, org, nx, ny, by, px, py, pair, n, w * h, prune, refine, hint)


def test_numbers_worked_out_by_hand():
    g = wg(496, 48)
    assert (g["items"], g["item_trips"], g["last_wave_lanes"]) == (510, 1, 62)
    g = wg(512, 48)
    assert (g["items"], g["item_trips"], g["last_wave_lanes"], g["wave_walk_trips"]) == (527, 2, 15, 2)
    assert (g["stage"], g["stage_total"], g["stage_trips"], g["stage_partial"]) == (1, 1536, 3, False)
    g = wg(512, 48, prune=1, hint=1)
    assert (g["stage"], g["stage_trips"], g["stage_clamped"], g["b1_lanes"], g["b1_idle"]) == (8, 1, True, 128, True)
    assert wg(512, 48, prune=1, hint=0)["stage"] == 1 and wg(512, 48, prune=1, hint=0)["b1_lanes"] == 0
    # quad loops
    assert [wg(w, 48, prune=1, hint=2)["b1_lanes"] for w in (272, 288)] == [64, 128]
    assert [wg(w, 50, 1, refine=True)["rq_lanes"] for w in (288, 304)] == [64, 128]
    assert [(wg(w, 48, prune=1, hint=1)["b1_lanes"], wg(w, 48, prune=1, hint=1)["b1_trips"]) for w in (2064, 2080)] == [(512, 1), (576, 2)]
    assert [(wg(w, 50, 1, refine=True)["rq_lanes"], wg(w, 50, 1, refine=True)["rq_trips"]) for w in (2080, 2096)] == [(512, 1), (576, 2)]
    assert wg(2064, 48)["last_wave_lanes"] == 0
    # staging borders: 48 chunks per 16 columns (50 less one with rows -1 and 32) against 4 096
    assert ref.PLAIN_BORDER == (1360, 1376) and ref.REFINE_BORDER == (1296, 1312)
    assert [wg(w, 48, prune=1, hint=1)["stage_total"] for w in ref.PLAIN_BORDER] == [4080, 4128]
    assert [wg(w, 50, 1, refine=True)["stage_total"] for w in ref.REFINE_BORDER] == [4049, 4099]
    assert all(wg(w, 48)["stage_partial"] and wg(w, 48, prune=1, hint=0)["stage_partial"] for w in ref.PLAIN_BORDER)
    # the pre-shift: floor-mod and floor-shift
    g = wg(320, 128, px=-17, by=3)
    assert (g["sh"], g["q16"], g["skip_left"], g["skip_right"]) == (15, -2, [0, 1], [])
    g = wg(320, 128, px=17, by=6)
    assert (g["sh"], g["q16"], g["skip_left"], g["skip_right"], g["tail_guard"], g["tail_bytes"]) == (1, 1, [], [17, 18], True, 15)
    assert g["reads"]["cur"][-1][1] == 320 * 128 - 1 and g["cur_chunks"] == 32 * 20 - 1
    assert not wg(320, 128, px=16, by=6)["tail_guard"] and not wg(320, 128, px=17, by=5)["tail_guard"]
    assert not wg(320, 130, 1, px=17, by=6)["tail_guard"], "the moved origin's last row and column absorb the over-read"
    g = wg(320, 128, py=-1, by=0)
    assert (g["rows_ok"], g["above"], g["items"], g["cur_chunks"], g["stage_total"]) == (False, True, 0, 0, 320)
    assert wg(320, 128, py=1, by=6)["below"] and wg(320, 128, py=1, by=5)["rows_ok"]
    # row 32 of the refining forms
    g = wg(160, 50, 1, by=1, pair=2, n=3, refine=True)
    assert (g["flat_chunks"], g["last_chunks"], g["odd"], g["pad_written"], g["row32_ends_on_last_byte"]) == (330, 9, 15, True, True)
    assert max(hi for _, hi in g["reads"]["cur"]) == 3 * 160 * 50 - 1
    assert not wg(160, 50, 1, by=1, pair=1, n=3, refine=True)["row32_ends_on_last_byte"]
    assert not wg(160, 64, 1, by=1, pair=2, n=3, refine=True)["row32_ends_on_last_byte"]
    assert wg(160, 50, 1, px=15, refine=True)["odd"] == 0 and wg(160, 50, 1, px=14, refine=True)["odd"] == 1
    # B2's list holds at most 16 rows of a block (B1 has done the 17th): 496 entries at nx 31 can never outgrow the 512 lanes
    assert 16 * 31 < ref.THREADS < 16 * 33


CENSUS = {   # every name paths() can return, and a device case that reaches it
    "form:plain:scan": "items-527", "form:plain:hint0": "items-527", "form:plain:hint1": "items-527", "form:plain:hint2": "items-527",
    "form:plain:hint3": "items-527", "form:plain:hint4": "items-527",
    "form:refine:scan": "items-527-half-pixel", "form:refine:hint0": "items-527-half-pixel", "form:refine:hint1": "items-527-half-pixel",
    "form:refine:hint2": "items-527-half-pixel", "form:refine:hint3": "items-527-half-pixel", "form:refine:hint4": "items-527-half-pixel",
    "preshift:none": "shifts-x", "preshift:displaced": "shifts-x", "shift16:-2": "shifts-x-half-pixel", "shift16:-1": "shifts-x",
    "shift16:0": "shifts-x", "shift16:1": "shifts-x",
    "rows:ok": "shifts-y", "rows:above-the-frame": "shifts-y", "rows:below-the-frame": "shifts-y",
    "skip:none": "shifts-x", "skip:left": "shifts-x", "skip:right": "shifts-x",
    "tail-guard:taken": "shifts-x", "tail-guard:not-needed": "items-527", "tail-guard:displaced-inside-the-frame": "shifts-x",
    "row32:odd-bytes": "ring-160x50", "row32:whole-chunks": "shifts-x-half-pixel", "row32:ends-on-the-last-byte": "ring-160x50",
    "pad:written": "ring-160x50", "pad:not-written": "shifts-y-half-pixel",
    "stage8:one-trip": "stage8-last-one-trip", "stage8:second-trip": "stage8-first-two-trips", "stage8:clamped-lanes": "stage8-last-one-trip",
    "stage1:partial-last-trip": "stage8-first-two-trips", "stage1:whole-trips": "items-527",
    "items:none": "shifts-y", "items:one-trip": "items-510", "items:second-trip": "items-527", "items:more-trips": "quads-128",
    "items:partial-wave": "items-527", "items:whole-waves": "quads-128",
    "b1:one-trip": "quads-128", "b1:second-trip": "quads-129", "b1:idle-quads": "quads-17", "b1:every-quad-a-block": "quads-16",
    "refine-loop:one-wave": "quads-16-half-pixel", "refine-loop:more-waves": "quads-17-half-pixel", "refine-loop:second-trip": "quads-129-half-pixel",
    "refine-loop:idle-quads": "quads-17-half-pixel", "refine-loop:every-quad-a-block": "quads-16-half-pixel",
    "place:one-block-row": "place-7x1", "place:more-block-rows": "place-5x2", "place:total-off-8": "place-9x1",
}


def all_paths(aof, orc, synth, c):
    out = set()
    for k in range(c["batches"]):
        out |= ref.paths(c, case_preds(aof, orc, synth, c, k), n_pairs=ref.batch_pairs(c, k))
    return out


def test_the_device_cases_reach_every_path_between_them(aof, orc, synth):
    """The census."""
    assert set(CENSUS) == set(ref.VOCABULARY) and len(ref.VOCABULARY) == len(set(ref.VOCABULARY))
    by_id = {c["id"]: c for c in ref.CASES}
    assert len(by_id) == len(ref.CASES) and all(c["why"] for c in ref.CASES)
    reached = {c["id"]: all_paths(aof, orc, synth, c) for c in ref.CASES}
    for name, cid in CENSUS.items():
        assert cid in by_id, f"the case {cid} that reaches {name} is gone"
        assert name in reached[cid], (name, cid, sorted(reached[cid]))
    assert set().union(*reached.values()) == set(ref.VOCABULARY)
    # the cases the issue names, at the widths it names
    widths = {(c["nx"], c["sub"]): c["w"] for c in ref.CASES if c["frames"] == "designed" and c["h"] in (48, 50)}
    for nx, w0, w1 in ((30, 496, 512), (31, 512, 528), (1, 32, 48), (16, 272, 288), (17, 288, 304), (128, 2064, 2080), (129, 2080, 2096)):
        assert (widths[(nx, 0)], widths[(nx, 1)]) == (w0, w1), nx
    assert widths[(2, 0)] == 48
    assert sorted((c["ny"], c["n_pairs"]) for c in ref.CASES if c["id"].startswith("place-")) == [(1, 1), (1, 3), (1, 7), (1, 9), (2, 3), (2, 5)]
    assert all((c["n_pairs"] * c["ny"]) % 8 for c in ref.CASES if c["id"].startswith("place-"))


def test_placement_is_a_permutation_of_every_launch():
    for c in ref.CASES:
        for k in range(c["batches"]):
            n = ref.batch_pairs(c, k)
            assert sorted(ref.placement(n, c["ny"])) == [(pair, by) for pair in range(n) for by in range(c["ny"])], c["id"]


def lds_of(w, h, org, prune, refine):
    return plan_ref.tile16_lds(plan_ref.t16("", w, h, subpixel=org, subdirs=int(refine), prune=prune))


def test_every_byte_read_lies_in_the_frame_arrays_and_every_lds_byte_in_the_allocation(aof):
    """The extents as a property: every width from 32 to 2 112, six heights (H % 16 in {0, 2}), both origins, every px in
    -17 .. 17, eight py, every block row, the first and the last pair of three.  The prev copy's 8 bytes into the next row,
    the displaced copy's sh bytes and g_flat[-1] are part of the extents."""
    n = 3
    px = np.arange(-17, 18).reshape(1, -1, 1, 1)
    py = np.array([-17, -16, -1, 0, 1, 15, 16, 17]).reshape(1, 1, -1, 1)
    pair = np.array([0, n - 1]).reshape(1, 1, 1, -1)
    swept = 0
    for w in range(32, 2112 + 1, 16):
        for h in (32, 34, 48, 50, 96, 98):
            for org in (0, 1):
                nx, ny = ref.grid(w, h, org)
                p = aof.default_params(w, h, tile=16, search=8, subpixel=org, min_valid=0)
                assert (aof.check_params(p) == 0) == (nx >= 1 and ny >= 1), (w, h, org)
                if nx < 1 or ny < 1:
                    continue
                g = aof.grid(p, 0)
                assert tuple(g) == (8 + org, 8 + org, 16, 16, nx, ny), (w, h, org, tuple(g))
                by = np.arange(ny).reshape(-1, 1, 1, 1)
                for refine in ((False, True) if org else (False,)):
                    e = ref.extents(w, h, org, by, px, py, pair, w * h, refine)
                    size = n * w * h
                    read = e["cur_hi"] >= e["cur_lo"]
                    assert (read == e["rows_ok"]).all()
                    where = lambda bad: (w, h, org, refine, np.argwhere(bad)[:4].tolist())
                    assert (e["cur_lo"][read] >= 0).all() and (e["cur_hi"][read] < size).all(), where(read & ((e["cur_lo"] < 0) | (e["cur_hi"] >= size)))
                    assert (e["prev_lo"] >= 0).all() and (e["prev_hi"] < size).all(), where((e["prev_lo"] < 0) | (e["prev_hi"] >= size))
                    for prune in (0, 1, 2):
                        L = ref.lds_layout(w, nx, prune, refine)
                        lds = lds_of(w, h, org, prune, refine)
                        assert (e["lds_lo"] >= 0).all() and (e["lds_hi"] < L["s_best"]).all() and L["end"] <= lds, (w, h, org, refine, prune, L, lds)
                    swept += e["cur_lo"].size
    assert swept == 3066560
    # the extents the sweep is there for are reached, not only allowed: the last byte of the arrays by both forms
    assert ref.extents(320, 128, 0, 6, 17, 0, 2, 320 * 128, False)["cur_hi"] == 3 * 320 * 128 - 1
    assert ref.extents(320, 130, 1, 6, 5, 0, 2, 320 * 130, True)["cur_hi"] == 3 * 320 * 130 - 1
    assert ref.extents(320, 130, 1, 0, 0, 0, 0, 320 * 130, True)["cur_lo"] == 0


def test_one_workgroup_in_full_agrees_with_the_swept_extents_and_stages_what_it_reads():
    """workgroup() on a coarser sweep (every px): its byte ranges have the extents' ends, do not overlap in LDS, every
    live window lies in its LDS row and in the moved frame, every ring byte of the refining forms was staged."""
    for w, h, org in ((48, 48, 0), (160, 96, 0), (320, 128, 0), (48, 50, 1), (160, 50, 1), (304, 98, 1), (320, 130, 1)):
        nx, ny = ref.grid(w, h, org)
        for refine in ((False, True) if org else (False,)):
            for px in range(-17, 18):
                for py in (-17, -16, -1, 0, 1, 15, 16, 17):
                    for by in range(ny):
                        for prune, hint in ((0, 0), (1, 1)):
                            g = ref.workgroup(w, h, org, nx, ny, by, px, py, 2, 3, w * h, prune, refine, hint)
                            e = ref.extents(w, h, org, by, px, py, 2, w * h, refine)
                            key = (w, h, org, refine, px, py, by)
                            cur = g["reads"]["cur"]
                            assert bool(cur) == bool(e["rows_ok"]), key
                            if cur:
                                assert (min(lo for lo, _ in cur), max(hi for _, hi in cur)) == (int(e["cur_lo"]), int(e["cur_hi"])), key
                            assert g["reads"]["prev"] == [(int(e["prev_lo"]), int(e["prev_hi"]))], key
                            spans = sorted(g["writes"])
                            assert spans[0][0] >= 0 and spans[-1][1] < lds_of(w, h, org, prune, refine), key
                            assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])), (key, spans)
                            assert (min(lo for lo, _ in spans[:-1]), max(hi for _, hi in spans[:-1])) == (int(e["lds_lo"]), int(e["lds_hi"])), key
                            assert g["tail_guard"] == bool(e["tail_guard"]) and g["sh"] == int(e["sh"])
                            for lo, hi in g["windows"]:
                                assert 0 <= lo and hi < w and hi + g["sh"] < w - 2 * org, (key, lo, hi)
                            if refine:
                                for lo, hi in g["ring"]:
                                    # (pad byte, rows -1 .. 31 and row 32's bytes lie end to end)
                                    assert g["staged"][0][0] <= lo and hi <= g["staged"][2][1], (key, lo, hi, g["staged"])


@pytest.mark.parametrize("c", ref.CASES, ids=lambda c: c["id"])
def test_the_grid_and_the_skipped_columns_are_the_products_and_the_oracles(aof, orc, synth, c):
    """nx, ny against aof.grid; the model's skipped blocks against the oracle's records with the feature gate off, under
    the oracle's own predictor."""
    for k in range(c["batches"]):
        p, prevs, curs, names, refs = oracle_of(aof, orc, synth, c, k, gate_off=True)
        g = aof.grid(p, 0)
        assert (g[4], g[5]) == (c["nx"], c["ny"]) and g[0] == 8 + c["org"] and prevs.shape[0] == ref.batch_pairs(c, k)
        for i, r in enumerate(refs):
            px, py = (int(r["flow"]["pred_x"]), int(r["flow"]["pred_y"])) if c["levels"] == 2 else (0, 0)
            want = np.zeros((c["ny"], c["nx"]), bool)
            for by in range(c["ny"]):
                w = ref.workgroup(c["w"], c["h"], c["org"], c["nx"], c["ny"], by, px, py, i, prevs.shape[0], c["w"] * c["h"], 0, bool(c["sub"]))
                want[by] = True
                want[by, w["live"]] = False
            got = (r["blocks"]["sad"] == 0xFFFF).reshape(c["ny"], c["nx"])
            assert np.array_equal(got, want), (c["id"], k, names[i], px, py, np.argwhere(got != want)[:6].tolist())


def test_the_predictor_cases_reach_what_they_are_there_for(aof, orc, synth):
    """Every px & 15, px >> 4 from -1 (-2 with half-pixel) to 1, windows out at both edges, block rows out above and below,
    the tail guard wherever the displaced copy ends on the frame's last byte -- from the oracle's flow records."""
    checked = 0
    for c in ref.CASES:
        if c["levels"] == 2:
            _, prevs, curs, _, refs = oracle_of(aof, orc, synth, c)
            rig.assert_predictor_census(c, rig.preds_of(refs), prevs, curs, ref)
            checked += 1
    assert checked == 5


def test_the_list_of_step_b2_outgrows_the_workgroup_where_the_case_says(aof, orc, synth):
    """From numpy sums of the oracle's SAD: on the unrelated-noise pair of the nx 33 case every verdict's list holds more
    than 512 entries in both block rows (bound_pays is evaluated), on the clean pair none does; at nx 31 the list cannot
    (16 x 31 = 496)."""
    for c in ref.CASES:
        if c["frames"] != "designed" or c["sub"] or c["nx"] not in (31, 33):
            continue
        p, prevs, curs, names, refs = oracle_of(aof, orc, synth, c)
        for i, name in enumerate(names):
            for hint in (1, 2, 3, 4):
                sizes, best = rig.b2_list_sizes(prevs[i], curs[i], c["nx"], c["ny"], hint)
                rec = refs[i]["blocks"]["sad"].reshape(c["ny"], c["nx"])
                assert (best[rec != 0xFFFF] == rec[rec != 0xFFFF]).all(), "the numpy SADs are the oracle's"
                if c["nx"] == 31:
                    assert max(sizes) <= 496
                elif name.startswith("unrelated"):
                    assert min(sizes) > ref.THREADS, (name, hint, sizes)
                elif name.startswith("clean"):
                    assert max(sizes) <= ref.THREADS, (name, hint, sizes)
    assert any(c.get("b2") for c in ref.CASES)
