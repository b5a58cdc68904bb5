"""The designed motion fields of tests/vote_field_ref.py against the oracle, on the CPU: for every named design at every
shape tests/test_gpu_vote_fields.py uses, orc.flow_pair on the generated pair votes exactly as designed, tile by tile;
orc.reduce on the designed records equals the pair's flow record; both equal reduce_model, byte for byte; and the
census of the oracle's records names the branches the design is there for.  These are conditions, not shares.  Then a
handful of cases whose expectations are literals worked out in their docstrings, the generator's refusals, and its
output pinned by sha256."""
import hashlib

import numpy as np
import pytest

import vote_field_ref as vf


def one_level_ids():
    return [(case, sub, name) for case, c in vf.ONE_LEVEL.items() for sub in c["size"] for name in vf.designs_of(case, sub)]


def same_bytes(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("case,sub,name", one_level_ids(), ids=lambda v: str(v))
def test_oracle_votes_as_designed(orc, case, sub, name):
    p = vf.one_level_params(orc.default_params, case, sub)
    g = orc.grid(p, 0)
    assert (g.x0, g.y0, g.step_x, g.step_y, g.nx, g.ny) == tuple(vf.grid_of(p)) and g.nx * g.ny == vf.ONE_LEVEL[case]["blocks"]
    assert orc.lib.orc_hist_size(p, 0) == vf.bins_of(p)
    cs = []
    for k, (d, prev, cur) in enumerate(vf.one_level_pairs(p, case, name)):
        r = orc.flow_pair(p, prev, cur)
        got = vf.design_of_records(p, r["blocks"], r["subdirs"])
        assert vf.same_field(p, d, got) == [], (case, sub, name, k)
        if name == "threshold":
            T, kind = vf.threshold_of(p), d.flat()[0]
            assert (r["blocks"]["sad"][kind == vf.SAD_BELOW] == T - 1).all() and (r["blocks"]["sad"][kind == vf.SAD_AT] == T).all()
            assert (kind == vf.SAD_BELOW).sum() >= 20 and (kind == vf.SAD_AT).sum() >= 20
        blocks, subdirs = vf.records_of_design(p, d)
        f, _, _ = orc.reduce(p, blocks, subdirs, vf.level_range(p))
        for field in ("flow_x", "flow_y", "count", "quality", "flags"):
            assert same_bytes(f[field], r["flow"][field]), (case, sub, name, k, field, f, r["flow"])
        assert same_bytes(vf.reduce_model(d, p), r["flow"]), (case, sub, name, k, vf.reduce_model(d, p), r["flow"])
        assert same_bytes(vf.reduce_model(got, p), r["flow"])
        cs.append(vf.census(got, p))
    vf.check_reaches(name, p, cs)


def test_the_one_level_cases_cover_every_tail_and_every_design():
    small = [c for c in vf.ONE_LEVEL.values() if c["blocks"] <= 256 and c["designs"] == vf.BUT_CHUNKS]
    assert {c["blocks"] % 4 for c in small} == {0, 1, 2, 3}
    assert set().union(*(c["designs"] for c in vf.ONE_LEVEL.values())) == set(vf.DESIGNS)
    assert vf.reduce_chunks(8320) == (3, 2774) and 8320 % 3 and vf.reduce_chunks(8192) == (0, 8192)


@pytest.mark.parametrize("hist_filter", [1, 0])
@pytest.mark.parametrize("field", sorted(vf.LEVEL1_FIELDS))
@pytest.mark.parametrize("case", sorted(vf.TWO_LEVEL))
def test_oracle_predictor_of_a_level1_field(orc, case, field, hist_filter):
    p = vf.two_level_params(orc.default_params, case, hist_filter=hist_filter)
    want = {"pred-2.5": [(-2, 3), (3, -2), (-2, 3)], "pred-3.5": [(-3, 4), (4, -3), (-3, 4)],
            "pred-3.0": [(-3, 3), (3, -3), (-3, 3)]}[field]
    for k, (d1, prev, cur) in enumerate(vf.level1_pairs(p, case, field)):
        r = orc.flow_pair(p, prev, cur, want_l1=True)
        got1 = vf.design_of_records(p, r["blocks_l1"], None, 1)
        assert vf.same_field(p, d1, got1) == [], (case, field, k)
        f = r["flow"]
        assert (int(f["pred_x"]), int(f["pred_y"])) == want[k] and f["flags"] & vf.FLAG_PRED_VALID, (case, field, k, f)
        c = vf.census(got1, p, 1)
        if field != "pred-3.0":
            assert c["pred_half_x"] and c["pred_half_y"], (case, field, k)
        got0 = vf.design_of_records(p, r["blocks"], None, 0)
        assert got0.voters().sum() > p.min_valid
        assert same_bytes(vf.pair_model(p, got0, d1), f), (case, field, k, vf.pair_model(p, got0, d1), f)
        b1, _ = vf.records_of_design(p, d1)
        _, px, py = orc.reduce(p, b1, None, vf.level_range(p, 1))
        assert (px, py) == want[k]


@pytest.mark.parametrize("name", vf.RESIDUALS)
@pytest.mark.parametrize("case", sorted(vf.TWO_LEVEL))
def test_oracle_votes_as_designed_under_a_predictor(orc, case, name):
    p = vf.two_level_params(orc.default_params, case)
    assert vf.bins_of(p) == orc.lib.orc_hist_size(p, 0) == vf.TWO_LEVEL[case].get("bins", 55)
    cs = []
    for k, (d0, P, prev, cur) in enumerate(vf.residual_pairs(p, case, name)):
        r = orc.flow_pair(p, prev, cur)
        f = r["flow"]
        assert (int(f["pred_x"]), int(f["pred_y"])) == P and f["flags"] & vf.FLAG_PRED_VALID, (case, name, k, P, f)
        got = vf.design_of_records(p, r["blocks"], None, 0)
        assert vf.same_field(p, d0, got) == [], (case, name, k)
        carriers = d0.voters() & (d0.vote != (2 * P[0], 2 * P[1])).any(2)
        assert 2 * carriers.sum() <= d0.kind.size
        assert same_bytes(vf.pair_model(p, d0, P=P), f), (case, name, k, vf.pair_model(p, d0, P=P), f)
        blocks, _ = vf.records_of_design(p, d0)
        g, _, _ = orc.reduce(p, blocks, None, vf.level_range(p))
        assert same_bytes(g["flow_x"], f["flow_x"]) and same_bytes(g["flow_y"], f["flow_y"]) and g["count"] == f["count"]
        cs.append(vf.census(got, p))
        assert cs[-1]["serial"] == ("bins" in vf.TWO_LEVEL[case])
    vf.check_reaches(name, p, cs)


# ---- literal expectations ----------------------------------------------------------------------------------------------
F = np.float32


def flow_of(orc, case, sub, name, variant):
    p = vf.one_level_params(orc.default_params, case, sub)
    d, prev, cur = vf.one_level_pairs(p, case, name)[variant]
    return p, d, orc.flow_pair(p, prev, cur)["flow"]


def test_hand_ends(orc):
    """84x84, half-pixel refinement: margin 5, 9 x 9 = 81 tiles, R = 4, centre 9, n = 19 bins.  `ends` variant 0: the x
    peak at bin 0 with its window's other bins 1, 2 and bin 3 outside; the y peak at bin 17 = n - 2 with 18, 16, 15 inside
    and 14 outside.  Groups (x bin, y bin): count -- (1, 18): 3, (2, 16): 2, (3, 15): 5, (0, 14): 4, and the other
    81 - 14 = 67 tiles on (0, 17).
    x: h[0] = 67 + 4 = 71, h[1] = 3, h[2] = 2, h[3] = 5.  Peak 0, window 0..2: sum k h = 3 + 4 = 7, sum h = 76.
    y: h[17] = 67, h[18] = 3, h[16] = 2, h[15] = 5, h[14] = 4.  Peak 17, window 15..18: 75 + 32 + 1139 + 54 = 1300, sum h
    = 77.  flow = (v / w - 9) / 2; all 81 vote: quality 255."""
    p, d, f = flow_of(orc, "b81", 1, "ends", 0)
    hx, hy, count = vf.histograms(d, p)
    assert hx[:5].tolist() == [71, 3, 2, 5, 0] and hy[13:].tolist() == [0, 4, 5, 2, 67, 3] and count == 81
    assert f["flow_x"] == (F(7) / F(76) - F(9)) / F(2) and f["flow_y"] == (F(1300) / F(77) - F(9)) / F(2)
    assert (f["count"], f["quality"], f["flags"]) == (81, 255, 1)


def test_hand_tie(orc):
    """84x84, integer votes: 81 tiles.  `tie` variant 0 around motion(4, 0) = (-2, -3) px: 37 tiles at dx = -2 (bin
    2 * -2 + 9 = 5), 37 at dx = 0 (bin 9), 3 at dx = -1 (bin 7), 4 silent; dy = -3 everywhere (bin 3).  The first maximum
    is bin 5; its window 3..7 holds bins 5 and 7: sum k h = 185 + 21 = 206, sum h = 40 (the last maximum, bin 9, would
    give 7..11: (21 + 333) / 40).  y: one bin, -3.  count 77, quality 77 * 255 // 81 = 242."""
    p, d, f = flow_of(orc, "b81", 0, "tie", 0)
    hx, hy, count = vf.histograms(d, p)
    assert (hx[5], hx[7], hx[9], hy[3], count) == (37, 3, 37, 77, 77)
    assert f["flow_x"] == (F(206) / F(40) - F(9)) / F(2) and f["flow_y"] == F(-3)
    assert f["flow_x"] != (F(354) / F(40) - F(9)) / F(2)
    assert (f["count"], f["quality"], f["flags"]) == (77, 242, 1)


def test_hand_spread(orc):
    """84x84, integer votes: 81 tiles.  `spread` variant 0 around (-1, -1) px (motion(4, 0) clipped to +-1 px, so that
    every group stays in range): x bins 5: 3, 9: 5, and outside the window 13: 4 and 3: 3; the peak, bin 7, has the other
    81 - 15 = 66 tiles less one that is silenced for an odd total: 65.  Window 5..9: sum k h = 15 + 455 + 45 = 515,
    sum h = 73.  y mirrors the small groups: bins 9: 3, 5: 5: 25 + 455 + 27 = 507 over 73.  Neither quotient is a dyadic
    fraction.  count 80, quality 80 * 255 // 81 = 251."""
    p, d, f = flow_of(orc, "b81", 0, "spread", 0)
    hx, hy, count = vf.histograms(d, p)
    assert (hx[3], hx[5], hx[7], hx[9], hx[13]) == (3, 3, 65, 5, 4) and (hy[5], hy[7], hy[9]) == (5, 65, 3) and count == 80
    assert f["flow_x"] == (F(515) / F(73) - F(9)) / F(2) and f["flow_y"] == (F(507) / F(73) - F(9)) / F(2)
    assert (f["count"], f["quality"], f["flags"]) == (80, 251, 1)


@pytest.mark.parametrize("field,pred", [("pred-2.5", (-2, 3)), ("pred-3.5", (-3, 4))])
def test_hand_predictor_halves(orc, field, pred):
    """96x80, two levels: level 1 is 48x40 with a 5 x 4 grid, R = 4, centre 9.  pred-2.5: 15 tiles at (-1, +1) and 5 at
    (-2, +2) level-1 px.  x: h[7] = 15, h[5] = 5: window 5..9, sum k h = 105 + 25 = 130 over 20 = bin 6.5, which is
    -2.5 half level-1 pixels = -2.5 level-0 pixels: floor((2 * 130 + 20) / 40) - 9 = 7 - 9 = -2, half up.  y: h[11] = 15,
    h[13] = 5: 230 / 20 = 11.5: floor(480 / 40) - 9 = +3.  pred-3.5 swaps the counts: 110 / 20 = 5.5 -> floor(240 / 40) - 9
    = -3, and 250 / 20 = 12.5 -> floor(520 / 40) - 9 = +4."""
    p = vf.two_level_params(orc.default_params, "c96")
    d1, prev, cur = vf.level1_pairs(p, "c96", field)[0]
    hx, hy, _ = vf.histograms(d1, p, 1)
    assert sorted(hx[hx > 0].tolist()) == [5, 15] and sorted(hy[hy > 0].tolist()) == [5, 15]
    f = orc.flow_pair(p, prev, cur)["flow"]
    assert (int(f["pred_x"]), int(f["pred_y"])) == pred and f["flags"] & vf.FLAG_PRED_VALID
    m = vf.reduce_model(d1, p, 1)
    assert (int(m["pred_x"]), int(m["pred_y"])) == pred


# ---- the generator itself ----------------------------------------------------------------------------------------------
def test_generator_refuses_what_cannot_come_out_as_designed(orc):
    p = orc.default_params(96, 80)
    g = vf.grid_of(p)
    ok = vf.Design.uniform(g.ny, g.nx, (2, -4))
    vf.make_pair(p, 0, ok)
    with pytest.raises(ValueError, match="half-pixel"):
        vf.make_pair(p, 0, vf.Design.uniform(g.ny, g.nx, (1, 0)))
    with pytest.raises(ValueError, match="range"):
        vf.make_pair(p, 0, vf.Design.uniform(g.ny, g.nx, (10, 0)))
    with pytest.raises(ValueError, match="design"):
        vf.make_pair(p, 0, vf.Design.uniform(g.ny + 1, g.nx))
    gated = vf.Design.uniform(g.ny, g.nx)
    gated.kind[0, 0] = vf.GATED
    with pytest.raises(ValueError, match="gate"):
        vf.make_pair(orc.default_params(96, 80, feature_threshold=0), 0, gated)
    with pytest.raises(ValueError, match="overlap"):      # the PX4Flow grid of a 40 x 40 frame steps by 4
        q = orc.px4flow_params(40, 40)
        vf.make_pair(q, 0, vf.Design.uniform(vf.grid_of(q).ny, vf.grid_of(q).nx))
    with pytest.raises(ValueError, match="two levels"):
        vf.make_pair(orc.default_params(96, 80, pyramid_levels=2), 0, ok)
    p2 = orc.default_params(96, 80, pyramid_levels=2)
    everywhere = vf.Design.uniform(g.ny, g.nx, (2, 2))
    with pytest.raises(ValueError, match="half of the tiles"):
        vf.make_pair(p2, 0, d0=vf.under_predictor(p2, everywhere, (-2, 2))[0], P=(-2, 2))


def test_only_the_tiles_of_prev_are_written(orc):
    p = vf.one_level_params(orc.default_params, "px4", 1)
    g = vf.grid_of(p)
    d = vf.design("uniform-random", g.ny, g.nx, 4, 0, True)
    prev, cur = vf.make_pair(p, 5, d)
    inside = np.zeros(prev.shape, bool)
    for j in range(g.ny):
        for i in range(g.nx):
            inside[g.y0 + j * g.step_y:g.y0 + j * g.step_y + 8, g.x0 + i * g.step_x:g.x0 + i * g.step_x + 8] = True
    assert np.array_equal(prev[~inside], cur[~inside]) and (prev[inside] != cur[inside]).any()
    assert np.array_equal(cur, vf.make_pair(p, 5, vf.design("one", g.ny, g.nx, 4, 1, True))[1])


PINS = [
    # (case, subpixel, design, variant, seed, sha256 of the design, sha256 of prev and cur)
    ("b108", 1, "quads", 1, 0, "27f95580a81ce66e68bb27729f71b740b00a5858f974b5012ba375f8d42a8401",
     "aae6b11d2bc1b3267bc2ee0127c7c6ad9a905465b700f0d5c9b2c129a01f7e1d"),
    ("b81", 0, "threshold", 0, 1, "8397872fca2ec516a3a766ab3d2c9709aa9c6d6ca64a78a7a46963eea63e2e39",
     "e23541d259b06bcd243e339263ce6700d53782b66278d150051257b628c40773"),
    ("px4", 1, "ends", 2, 2, "a749ca506c7157f62cb57f42da4fa4f7a0267e714a64679d857e218fef6c0d3a",
     "e449ce601b5ab310547ec5cb75a7cdf2407f123cffa6c7f4c811af01a7344c28"),
]


@pytest.mark.parametrize("k", range(len(PINS)), ids=[f"{e[2]}-seed{e[4]}" for e in PINS])
def test_generator_output_is_pinned(orc, k):
    case, sub, name, variant, seed, want_design, want_frames = PINS[k]
    p = vf.one_level_params(orc.default_params, case, sub)
    g = vf.grid_of(p)
    d = vf.design(name, g.ny, g.nx, 4, variant, bool(sub) and name != "threshold")
    prev, cur = vf.make_pair(p, seed, d)
    assert prev.dtype == cur.dtype == np.uint8
    assert d.digest() == want_design
    assert hashlib.sha256(prev.tobytes() + cur.tobytes()).hexdigest() == want_frames


def test_two_level_generator_output_is_pinned(orc):
    p = vf.two_level_params(orc.default_params, "c96")
    _, prev, cur = vf.level1_pairs(p, "c96", "pred-2.5", seed=3)[0]
    assert hashlib.sha256(prev.tobytes() + cur.tobytes()).hexdigest() == \
        "a122939e793b19db49849b255398127b98355603fabf5ecd2542faa3be6916b5"
    _, _, prev, cur = vf.residual_pairs(p, "c96", "tie", seed=4)[1]
    assert hashlib.sha256(prev.tobytes() + cur.tobytes()).hexdigest() == \
        "cf9b26b464d366f887ec1fdaddad1629c547848f05cddbf09da593b66dcdd63d"
