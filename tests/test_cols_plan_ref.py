"""The column walk's plan without a device (tests/cols_plan_ref.py): the model's plan at every boundary worked out by hand,
the kernel's unit decode on every case -- each block of each pair written by exactly one lane, no wave across two pairs or
two segment classes, no pair index beyond the launch, every unit below 31 bits --, every case held to the paths it is
listed for, and the census: a path of the vocabulary that no DEVICE case takes fails here.  The same plans come out of
the C++ function in tests/test_host_asan.py."""
import numpy as np
import pytest

import cols_plan_ref as ref

EVERY_CASE = ref.CPU_CASES + ref.GPU_CASES


def test_the_plan_at_the_boundaries_worked_out_by_hand():
    def short(nx, ny, n, **kw):
        p = ref.plan(nx, ny, n, **kw)
        return p["head"]["len"], p["tail"]["len"], p["tail_pairs"], p["head_pairs"], p["head_units"], p["units"], p["wgs"]

    # 17 x 16, eight rows: 2 segments x 17 columns = 34 units, one wave per pair; four rows: 4 x 17 = 68, two waves
    # 3 071 pairs: five rows (4 x 17 = 68 units in 128), 6 142 waves, rest 2 046 = 1 023 pairs; the tail's two rows: 8 x 17 = 136 in 192
    assert short(17, 16, 3071) == (5, 2, 1023, 2048, 2048 * 128, 2048 * 128 + 1023 * 192, (2048 * 128 + 1023 * 192 + 255) // 256)
    assert short(17, 16, 3072)[:4] == (8, 4, 0, 3072)
    assert short(17, 16, 4096)[:4] == (8, 4, 0, 4096)                 # all == kWaveSlots
    assert short(17, 16, 4097) == (8, 4, 1, 4096, 4096 * 64, 4096 * 64 + 128, 1025)
    assert short(17, 16, 4096 + 3276)[2] == 3276 and short(17, 16, 4096 + 3277)[2] == 0   # rest * 5 < 16 384
    assert short(17, 16, 8192)[2] == 0 and short(17, 16, 8191)[2] == 0 and short(17, 16, 8193)[2] == 1
    # 65 x 6 at 1 400 pairs: five rows, 2 x 65 = 130 units in 192; tail of two rows, 3 x 65 = 195 in 256
    assert short(65, 6, 1400) == (5, 2, 35, 1365, 1365 * 192, 1365 * 192 + 35 * 256, (1365 * 192 + 35 * 256 + 255) // 256)
    assert short(65, 6, 1365)[2:4] == (0, 1365) and short(65, 6, 1366)[2:4] == (1, 1365)   # 4 095 / 4 098 waves
    # the tables of the issue
    assert [short(65, ny, 1400)[:3] for ny in range(4, 10)] == [(3, 2, 35), (4, 2, 35), (5, 2, 35), (6, 3, 35), (7, 3, 35), (8, 4, 35)]
    assert short(17, 16, 2100)[:4] == (5, 2, 52, 2048) and short(100, 5, 1100)[:4] == (4, 2, 76, 1024)
    assert short(23, 19, 1400)[:3] == (3, 2, 35)
    # clipped to the grid's rows
    assert short(65, 5, 2100)[:4] == (5, 4, 52, 2048) and short(87, 3, 2100)[:3] == (3, 3, 0) and short(130, 2, 1500)[:3] == (2, 2, 0)
    # the 600-pair VGA launch of tests/test_gpu_parity.py: head 8, tail 4
    assert short(79, 59, 600)[:4] == (8, 4, 191, 409)   # 8 x 79 = 632 units in 640: 6 000 waves, rest 1 904
    # aligned: every condition by itself
    ok = dict(w=528, h=56)
    assert ref.plan(65, 6, 9, **ok)["aligned"] == 1
    for kw in (dict(w=530, h=56), dict(w=529, h=56), dict(ok, pair_stride=528 * 56 + 2), dict(ok, cur=1), dict(ok, cur=2), dict(ok, step_x=9),
               dict(w=530, h=57, pair_stride=530 * 57 + 2)):
        assert ref.plan(65, 6, 9, **kw)["aligned"] == 0, kw
    assert ref.plan(65, 6, 9, **dict(ok, cur=0x7F00DEAD0004, pair_stride=528 * 56 + 4))["aligned"] == 1
    # pairs per launch: units stay below 31 bits
    p = ref.plan(17, 16, 0x7FFF0000 // 128 + 5)                       # (the tail's four rows: 4 x 17 = 68 units in 128)
    assert p["per"] == 0x7FFF0000 // 128 and p["n_pairs"] == p["per"] and p["units"] <= 0x7FFF0000
    assert ref.plan(17, 16, 0x7FFF0000 // 128 + 5, done=p["per"])["n_pairs"] == 5


def test_fast_div_of_the_model():
    rng = np.random.default_rng(1)
    for d in list(range(1, 300)) + [64 * k for k in (5, 77, 1000, 16384)] + [4095, 4096, 4097]:
        fd = ref.fastdiv_make(d)
        n = np.concatenate([np.arange(0, 5000, dtype=np.uint64), rng.integers(0, 0x7FFFFFFF, 5000).astype(np.uint64),
                            np.array([0x7FFEFFFF, 0x7FFFFFFF], dtype=np.uint64)])
        assert (ref.fast_div(n, fd) == n // np.uint64(d)).all(), d


@pytest.mark.parametrize("c", EVERY_CASE, ids=lambda c: c["id"])
def test_the_decode_writes_every_block_once(c):
    pl = ref.plan_of(c)
    assert pl["units"] < 0x7FFF0000 and pl["wgs"] * ref.THREADS < 2 ** 31
    assert pl["head_units"] == pl["head_pairs"] * pl["head"]["units_per_pair"] and pl["head_units"] % 64 == 0
    d = ref.decode(pl)
    # no wave holds two classes or two pairs: what every lane computes for itself is what the first lane computed
    assert (d["lane_class"] == d["in_tail"]).all()
    assert (d["lane_pair"] == d["pair"]).all()
    # waves beyond the launch's units leave; every other wave has a pair of the launch
    beyond = d["unit0"] >= np.uint64(pl["units"])
    assert (d["returns"] == beyond).all()
    assert (d["pair"][~d["returns"]] < pl["n_pairs"]).all() and (d["pair"][~d["returns"]] >= 0).all()
    # head pairs walk head segments, tail pairs tail segments
    walks = ~d["returns"]
    assert ((d["pair"][walks] >= pl["head_pairs"]) == d["in_tail"][walks]).all()
    assert (d["bx"][walks & d["live"]] < pl["nx"]).all() and (d["by0"][walks & d["live"]] < pl["ny"]).all()
    cover = ref.coverage(pl, d)
    assert cover.shape == (pl["n_pairs"], pl["ny"], pl["nx"])
    assert (cover == 1).all(), np.argwhere(cover != 1)[:8]


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_every_device_case_reaches_the_paths_it_is_listed_for(c):
    assert c["paths"], "a case without a path has no reason to be in the list"
    got = ref.reach(c)
    assert set(c["paths"]) <= set(ref.VOCABULARY), set(c["paths"]) - set(ref.VOCABULARY)
    assert set(c["paths"]) <= got, (c["id"], sorted(set(c["paths"]) - got))
    assert got <= set(ref.VOCABULARY), got - set(ref.VOCABULARY)
    assert c["w"] * c["h"] * 2 * c["n_pairs"] <= 125 * 10 ** 6


def test_the_device_cases_reach_every_path_between_them():
    """The census."""
    reached = set()
    for c in ref.GPU_CASES:
        reached |= ref.reach(c)
    claimed = {name for c in ref.GPU_CASES for name in c["paths"]}
    missing = set(ref.VOCABULARY) - reached
    assert missing == set(ref.UNREACHABLE), f"paths no device case reaches: {sorted(missing - set(ref.UNREACHABLE))}"
    assert len(ref.UNREACHABLE) == 1 and all(ref.UNREACHABLE.values())
    assert claimed <= reached
    assert len({c["id"] for c in EVERY_CASE + ref.PLAN_ONLY}) == len(EVERY_CASE + ref.PLAN_ONLY)
    # the second launch of a call is the unreachable one: the first holds more frames than the device has memory (288 GB)
    for nx, ny in ((17, 16), (16, 17), (65, 4), (79, 59), (159, 119)):
        for n in (1, 10 ** 7):
            assert ref.plan(nx, ny, n)["per"] * 2 * (8 * nx + 8) * (8 * ny + 8) > 288 * 2 ** 30, (nx, ny, n)


def test_the_plan_only_cases_are_the_split_into_launches():
    first, second, exact, larger = (ref.plan_of(c) for c in ref.PLAN_ONLY)
    assert first["n_pairs"] == first["per"] and second["n_pairs"] == 5 and exact["n_pairs"] == exact["per"]
    assert larger["tail"]["units_per_pair"] > larger["head"]["units_per_pair"] and larger["n_pairs"] == larger["per"] == 0x7FFF0000 // 192
    for p in (first, second, exact, larger):
        assert p["units"] <= 0x7FFF0000


def modal(q):
    """The most frequent (dx, dy) of block records."""
    m, n = np.unique(np.stack([q["dx"], q["dy"]], 1), axis=0, return_counts=True)
    return tuple(m[n.argmax()])


def share(q, m):
    """The fraction of block records with motion m."""
    return ((q["dx"] == m[0]) & (q["dy"] == m[1])).mean()


@pytest.mark.parametrize("c", ref.GPU_CASES, ids=lambda c: c["id"])
def test_the_frames_of_a_device_case_are_what_the_case_says(aof, orc, synth, c):
    """The parameter check takes the frame, the grid is the case's, the predictors are the listed ones (reach() derives the
    misalignments from them), every two-level pair has a delta, the flat pair is gated everywhere, the split pair holds
    two motions and the noise pair votes all over the histogram."""
    p = aof.default_params(c["w"], c["h"], **ref.params_kw(c))
    assert aof.check_params(p) == 0
    g = aof.grid(p, 0)
    assert (g[2], g[3], g[4], g[5]) == (8, 8, c["nx"], c["ny"]) and g[0] == 4 + c["subpixel"]
    prevs, curs = ref.pairs_for(c, synth)
    k = ref.distinct_pairs(c)
    assert prevs.shape == (k, c["h"], c["w"]) and ref.case_plan(c)["head_pairs"] % k != 0 and 6 <= k <= 8
    out = [orc.flow_pair(orc.params_from(p), prevs[i], curs[i]) for i in range(k)]
    if c["levels"] == 2:
        assert tuple(int(o["flow"]["pred_x"]) for o in out) == c["px"][:k]
        assert all(ref.delta_of(c, prevs[i], curs[i]) != 0 for i in range(k))
        assert {px & 3 for px in c["px"][:k]} == {0, 1, 2, 3}
    else:
        assert c["px"] == ()
    assert (out[2]["blocks"]["sad"] == 0xFFFF).all() and out[2]["flow"]["count"] == 0
    b = out[1]["blocks"].reshape(c["ny"], c["nx"])
    top, bottom = b[:c["ny"] // 2], b[(c["ny"] + 1) // 2:]
    top, bottom = top[top["sad"] != 0xFFFF], bottom[bottom["sad"] != 0xFFFF]
    assert top.size and bottom.size and min(share(bottom, modal(top)), share(top, modal(bottom))) < 0.5
    noise = out[3]["blocks"][out[3]["blocks"]["sad"] < p.value_threshold]
    assert noise.size > 100 and np.unique(noise["dx"]).size >= 7 and np.unique(noise["dy"]).size >= 7
    if c["subpixel"]:
        assert set(np.unique(out[4]["subdirs"]).tolist()) - {8}, "the half-pixel pair refines somewhere"
