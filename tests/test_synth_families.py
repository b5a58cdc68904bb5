"""The camera-like input families of synth.py (natural, lowtex, warp, subpel, vignette and the camera sequence):
their bytes are pinned, each has the property it exists for, and on each the oracle agrees with the independent
numpy restatement (npref.py), as test_oracle_matches_numpy_restatement shows for the box texture.  The generators
that the goldens, the hand vectors and bench.py rest on are pinned too: adding families must not move a byte."""
import hashlib

import numpy as np
import pytest

import npref


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def pdict(p):
    return {n: getattr(p, n) for n, _ in p._fields_}


# ---- pins ------------------------------------------------------------------------------------------------------------

EXISTING = [
    ("make_pair", (64, 48, 4, 0), {}, "07d0374dcd57f21888f92e2d4ae3adda598e8de04e305a9e13b68cf72e061438"),
    ("make_pair", (96, 64, 4, 7), dict(noise=3, brightness=9),
     "d5e9c564f104811a6632d1c3cbaec4ec72bb0098b1aa335448304e5388993263"),
    ("make_pair", (80, 80, 8, 123), dict(half=(1, -1), shift=(3, -2), contrast=2.0),
     "dc0a97b447456fb213f8798c8f5c8f3e19afca9948316c6b23c94b3ba811ede4"),
    ("make_batch", (64, 48, 3), {}, "6c4d61d92be9c2168f32494d6cb8cc998ef74f39332e38de9555fb87ccb6f799"),
    ("make_batch", (96, 64, 2, 4, 100), dict(noise=2), "19880e0c84c4cc6d858d7ba5f3094dfd0069a83d4c1de1842ce0c5626d658bdb"),
    ("make_batch", (128, 96, 2, 9, 8100), dict(brightness=-20),
     "02c5f4324f0a5edeb345d9043c269833bae9c257e9c69ed12e7be6627000b9d4"),
    ("make_sequence", (64, 48, 4), {}, "76d3b19f15cbd81a16f10f059a157a92cb982ca1513adcad7175591857a6f984"),
    ("make_sequence", (96, 64, 5, 4, 3), {}, "de0688062375d386d7214dbfb05269126e8ec6c2b0dc5c70c05b3b4fb58bba4e"),
    ("make_sequence", (128, 96, 3, 8, 11, 2), {}, "b946b235f1b1d88e8d807cf7035391dbf85178fa7cf804d25f225e0df31a0e65"),
]


@pytest.mark.parametrize("k", range(len(EXISTING)), ids=[f"{e[0]}-{i}" for i, e in enumerate(EXISTING)])
def test_existing_generators_are_unchanged(synth, k):
    name, args, kw, want = EXISTING[k]
    out = getattr(synth, name)(*args, **kw)
    if name == "make_pair":
        out = (out[0], out[1], np.array(out[2]))
    assert digest(*out) == want


FAMILY_PINS = [
    # (family, (width, height, reach, pair_index, noise), keyword arguments, sha256 of prev, cur and the exact truth)
    ("natural", (96, 64, 4, 0, 0), dict(alpha=1.0),
     "bbde2459ecf8c71bf45aa0c00439ffeba811a5e8e57f6d63ea8f4977a5c04320"),
    ("natural", (96, 64, 4, 1, 4), dict(alpha=1.5),
     "e7ff190ba76fefc7da8ac3108a0fc437a5997281550406be6af9eb7cbf88e0ac"),
    ("lowtex", (96, 64, 4, 0, 0), {},
     "a1a862cd00f51379bebd01399972231b9eb2fb9a56f9455261630651b90d21b7"),
    ("lowtex", (128, 96, 8, 3, 16), {},
     "4ca615d5cb33bcf130a638a23a6c0aea16a64586cdb093ffe839b980be618b5f"),
    ("warp", (96, 64, 4, 0, 0), dict(preset="zoom_in_2"),
     "db47f4eaec6cc27e9908c1e8f4a38bd555975c80d6c0dfa53acfc6dc547ec4db"),
    ("warp", (96, 64, 4, 1, 4), dict(preset="zoom_out_1"),
     "c8f6a02e0bc778418f511434350734df96699fc4be8a8b5c86434bedf8b7e02d"),
    ("warp", (96, 64, 4, 2, 0), dict(preset="rotate_2"),
     "572e57120ed39bd5956b3f4a882a0b8ca2e57f04c4ac6cbd04d8e7450a9c5392"),
    ("warp", (96, 64, 4, 3, 16), dict(preset="rotate_m1"),
     "a33bf1a038d57321a61d9761c70ee0f49d689f08089029bea3f2a86d56e07fe3"),
    ("warp", (96, 64, 4, 4, 0), dict(preset="zoom_rotate"),
     "4fbbe35563b50bba9565e3496b57dd92130f4549d807872909a53f0f5cb3c005"),
    ("subpel", (96, 64, 4, 0, 0), {},
     "39c74c264f286ba304a4d3601475578d98a51c62dfacc167f5825336bcff5b8c"),
    ("subpel", (96, 64, 4, 5, 4), {},
     "16b6db038778a3afad514e4df58e76cf1156f88ea6c46ff690cdcc977c990d5b"),
    ("vignette", (96, 64, 4, 0, 0), {},
     "768c6af82da242cc3b9300b8991aea02d40a5bdbeb47f6102ff7df9f5298f966"),
    ("vignette", (96, 64, 4, 1, 4), {},
     "f0c2762b29654379cc3dd5b587a004ad831a15d0e1ffd52d5358698a90c5af74"),
    ("vignette", (96, 64, 4, 2, 0), {},
     "2b32e1f109798bd3f7ae3be39aba36fc47b30ed6a9f62c6c77f1acb1820cf28c"),
    ("vignette", (96, 64, 4, 3, 16), {},
     "530eaf9d2d7c90002b13ecb5e5f9d432fbff7285d3c7fa9b6a11c3aa166f11d6"),
    ("terrace", (96, 64, 4, 0, 0), {},
     "caab8d600d68102d63909944d27cda350ec4ee8d0394b571cb3e4f5634f89999"),
    ("terrace", (96, 64, 4, 1, 0), {},
     "dbf2cc11cec4b6852daf5f6aef924b5c4f7c8c5bbb19df58fd0943d5e15989f6"),
    ("terrace", (128, 96, 8, 2, 4), {},
     "28c741227c5df4f075c54284bab3c6877b25e02906154108837f40fa979efd27"),
]
CAMERA_PIN = "af2c23cdcc98c355ac37aab2df945589ba5de5b17dfae660d48467b87daa0d49"


def family_digest(synth, family, args, kw):
    prev, cur, truth = synth.make_family_pair(family, *args, **kw)
    if family == "warp":   # (the field is computed in floating point; the pixels are not)
        return digest(prev, cur)
    if family == "terrace":
        return digest(prev, cur, truth)
    return digest(prev, cur, np.array(truth, dtype=np.float64))


@pytest.mark.parametrize("k", range(len(FAMILY_PINS)), ids=[f"{e[0]}-{i}" for i, e in enumerate(FAMILY_PINS)])
def test_family_presets_are_pinned(synth, k):
    family, args, kw, want = FAMILY_PINS[k]
    assert family_digest(synth, family, args, kw) == want


def test_camera_sequence_is_pinned(synth):
    frames, pos = synth.make_camera_sequence(96, 64, 5, seed=0)
    assert digest(frames, pos) == CAMERA_PIN


# ---- properties --------------------------------------------------------------------------------------------------------

def spectrum_slope(img, lo=0.01, hi=0.25):
    """Log-log slope of the radially averaged amplitude spectrum over [lo, hi] cycles per pixel."""
    f = np.abs(np.fft.fft2(img.astype(np.float64) - img.mean()))
    fy = np.fft.fftfreq(img.shape[0])[:, None]
    fx = np.fft.fftfreq(img.shape[1])[None, :]
    r = np.hypot(fx, fy)
    edges = np.geomspace(lo, hi, 17)
    xs, ys = [], []
    for a, b in zip(edges[:-1], edges[1:]):
        ring = (r >= a) & (r < b)
        xs.append(np.log(np.sqrt(a * b)))
        ys.append(np.log(f[ring].mean()))
    return float(np.polyfit(xs, ys, 1)[0])


@pytest.mark.parametrize("alpha", [1.0, 1.5])
def test_natural_spectrum_falls_as_one_over_f_to_the_alpha(synth, alpha):
    for k in range(2):
        prev, cur, _ = synth.make_natural_pair(640, 480, 4, k, alpha=alpha)
        for img in (prev, cur):
            s = spectrum_slope(img)
            assert abs(s + alpha) <= 0.35, (alpha, k, s)


def gate_fail_fraction(orc, img, tile, search):
    p = orc.default_params(img.shape[1], img.shape[0], tile=tile, search=search)
    g = orc.grid(p, 0)
    d = [orc.compute_diff(img, g.x0 + bx * g.step_x, g.y0 + by * g.step_y, tile)
         for by in range(g.ny) for bx in range(g.nx)]
    return float(np.mean(np.array(d) < p.feature_threshold))


def test_lowtex_fails_the_gate_on_about_half_of_the_tiles(orc, synth):
    assert orc.default_params(640, 480).feature_threshold == 30
    for k in range(2):
        f8 = gate_fail_fraction(orc, synth.make_lowtex_pair(640, 480, 4, k)[0], 8, 4)
        assert 0.35 <= f8 <= 0.65, (k, f8)
    f16 = gate_fail_fraction(orc, synth.make_lowtex_pair(1280, 960, 8, 0)[0], 16, 8)
    assert 0.35 <= f16 <= 0.65, f16


def block_truth(orc, p, truth):
    """The warp's displacement at the centre pixel of every block of the level-0 grid, [ny, nx, 2]."""
    g = orc.grid(p, 0)
    c = p.tile // 2
    ys = g.y0 + np.arange(g.ny) * g.step_y + c
    xs = g.x0 + np.arange(g.nx) * g.step_x + c
    return truth[ys[:, None], xs[None, :]]


@pytest.mark.parametrize("preset", ["rotate_2", "rotate_m1", "zoom_in_2", "zoom_out_1", "zoom_rotate"])
def test_warp_records_follow_the_field_and_change_down_the_columns(orc, synth, preset):
    p = orc.default_params(640, 480)
    prev, cur, truth = synth.make_warp_pair(640, 480, 4, 3, preset=preset)
    assert truth.shape == (480, 640, 2)
    r = orc.flow_pair(p, prev, cur)
    g = orc.grid(p, 0)
    b = r["blocks"].reshape(g.ny, g.nx)
    t = block_truth(orc, p, truth)
    live = b["sad"] != 0xFFFF
    inside = live & (np.abs(t[..., 0]) <= p.search) & (np.abs(t[..., 1]) <= p.search)
    assert inside.mean() >= 0.15, inside.mean()
    near = (np.abs(b["dx"] - np.rint(t[..., 0])) <= 1) & (np.abs(b["dy"] - np.rint(t[..., 1])) <= 1)
    assert (near & inside).sum() >= 0.9 * inside.sum(), ((near & inside).sum(), inside.sum())
    changed = (b[1:]["dx"] != b[:-1]["dx"]) | (b[1:]["dy"] != b[:-1]["dy"])
    assert changed.mean() >= 0.10, changed.mean()


def test_subpel_half_pixel_pair_takes_every_direction(orc, synth):
    p = orc.default_params(640, 480, subpixel=1)
    prev, cur, truth = synth.make_subpel_pair(640, 480, 4, 0)
    assert truth[0] % 1 == 0.5 and truth[1] % 1 == 0.5, truth
    r = orc.flow_pair(p, prev, cur)
    assert set(np.unique(r["subdirs"]).tolist()) == set(range(9)), np.bincount(r["subdirs"], minlength=9)


def test_subpel_truth_is_the_bilinear_shift(synth):
    """A quarter-pixel shift of (4, -8) quarters is a whole-pixel crop: cur(x, y) = prev(x - 1, y + 2)."""
    prev, cur, truth = synth.make_subpel_pair(96, 64, 4, 2, quarter=(4, -8))
    assert truth == (1.0, -2.0)
    assert np.array_equal(cur[:-2, 1:], prev[2:, :-1])


def test_vignette_equalisation_clamps_at_both_ends(orc, synth):
    ends = set()
    for k in range(len(synth.VIGNETTE_STEPS)):
        prev, cur, _ = synth.make_vignette_pair(640, 480, 4, k)
        d = orc.frame_mean(prev) - orc.frame_mean(cur)
        raw = cur.astype(np.int64) + d
        assert np.array_equal(orc.equalise(cur, d), np.clip(raw, 0, 255))
        low, high = float(np.mean(raw < 0)), float(np.mean(raw > 255))
        assert max(low, high) >= 0.01, (k, d, low, high)
        ends.add("0" if low >= 0.01 else "255")
    assert ends == {"0", "255"}


def test_terrace_puts_blocks_on_the_bounds(orc, synth):
    """With the gate off: blocks whose every candidate ties at SAD 0, best SADs of a few LSB, and half-pixel directions
    chosen by a few LSB; the records of textured blocks follow their stripe's shift."""
    p = orc.default_params(640, 480, subpixel=1, feature_threshold=0, value_threshold=70000)
    for k, (want_zero, want_small) in enumerate(((0.5, 0.0), (0.0, 0.05), (0.0, 0.05))):
        prev, cur, truth = synth.make_terrace_pair(640, 480, 4, k)
        assert set(np.unique(prev).tolist()) == set(range(125, 131))
        r = orc.flow_pair(p, prev, cur)
        s = r["blocks"]["sad"]
        assert (s == 0).mean() >= want_zero and ((s > 0) & (s <= 16)).mean() >= want_small, (k, np.bincount(s)[:20])
        if k:
            assert (r["subdirs"] != 8).sum() >= 50, (k, np.bincount(r["subdirs"], minlength=9))
    prev, cur, truth = synth.make_terrace_pair(640, 480, 4, 3, half=(0, 0))
    p = orc.default_params(640, 480)
    g = orc.grid(p, 0)
    b = orc.flow_pair(p, prev, cur)["blocks"].reshape(g.ny, g.nx)
    t = block_truth(orc, p, truth)
    live = b["sad"] != 0xFFFF
    exact = (b["dx"] == t[..., 0]) & (b["dy"] == t[..., 1]) & (b["sad"] == 0)
    assert live.sum() >= 100 and (exact & live).sum() >= 0.8 * live.sum(), ((exact & live).sum(), live.sum())


def test_camera_sequence_pans_and_zooms(orc, synth):
    frames, pos = synth.make_camera_sequence(320, 240, 5, seed=3)
    p = orc.default_params(320, 240)
    g = orc.grid(p, 0)
    for k in range(4):
        b = orc.flow_pair(p, frames[k], frames[k + 1])["blocks"].reshape(g.ny, g.nx)
        centre = b[g.ny // 2 - 2:g.ny // 2 + 2, g.nx // 2 - 2:g.nx // 2 + 2]
        step = pos[k + 1] - pos[k]
        assert np.median(centre["dx"]) == -step[0] and np.median(centre["dy"]) == -step[1], (k, step)
        # the zoom: the rim moves away from the centre
        assert np.median(b[:, -4:]["dx"]) > np.median(b[:, :4]["dx"])


# ---- the oracle against the numpy restatement on every family -------------------------------------------------------

GEOMETRIES = {
    "8x8-64x64": (dict(width=64, height=64), 4),
    "8x8-96x64": (dict(width=96, height=64), 4),
    "two-level-eq": (dict(width=96, height=64, pyramid_levels=2, mean_subtract=1), 9),
    "px4-half-pixel": (dict(width=64, height=64, grid_mode=1, num_blocks=5, subpixel=1), 4),
    "16x16-80x80": (dict(width=80, height=80, tile=16, search=8, value_threshold=12000), 8),
}


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("family", ["natural", "lowtex", "warp", "subpel", "vignette", "terrace"])
def test_oracle_matches_numpy_restatement_on_family(orc, synth, family, geometry):
    kw, reach = GEOMETRIES[geometry]
    p = orc.default_params(**kw)
    for trial, noise in enumerate((0, 4)):
        kw = dict(alpha=(1.0, 1.5)[trial]) if family == "natural" else {}
        prev, cur, _ = synth.make_family_pair(family, p.width, p.height, reach, 11 + trial, noise, **kw)
        r = orc.flow_pair(p, prev, cur)
        n = npref.flow_pair(pdict(p), prev, cur)
        recs = [(int(b["dx"]), int(b["dy"]), int(b["sad"])) for b in r["blocks"]]
        assert recs == n["recs"], (family, geometry, trial)
        assert list(r["subdirs"]) == n["subs"], (family, geometry, trial)
        f = r["flow"]
        assert f["flow_x"] == n["flow_x"] and f["flow_y"] == n["flow_y"]
        assert f["count"] == n["count"] and f["quality"] == n["quality"]
        assert (f["pred_x"], f["pred_y"]) == (n["pred_x"], n["pred_y"])
        assert bool(f["flags"] & 1) == n["valid"] and bool(f["flags"] & 2) == n["pred_valid"]
