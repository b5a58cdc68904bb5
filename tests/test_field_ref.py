"""The motion-field fit on the CPU (include/aof.h, "the motion FIELD of a batch"): hand literals on the 64x64 dense grid,
outliers and degenerate inputs, the edges of the acceptance rule, aof_field_host against the numpy model (tests/field_ref.py)
byte for byte on every geometry the kernel is held to, the ABI and its refusals, and what the fit is FOR: on zooming and
rotating pairs (synth.make_warp_pair, the oracle's records) the fitted centre flow, zoom and rotation against the truth,
where the histogram flow of the same records misses by half a pixel and more."""
import ctypes as C
import functools

import numpy as np
import pytest

import field_ref as fr
import vote_field_ref as vf


def p64(aof, **kw):
    return aof.default_params(64, 64, **kw)


def flows_of(n, pred=(0, 0)):
    f = np.zeros(n, fr.FLOW_DTYPE)
    f["pred_x"], f["pred_y"] = pred
    return f


def both(aof, p, blocks, subdirs, flow=None, **kw):
    """The host function's record, which must be the model's byte for byte."""
    flows = flows_of(1) if flow is None else flow
    got = aof.field_host(p, blocks[None], flows, None if subdirs is None else subdirs[None], aof.field_params(**kw))
    want = fr.model(p, blocks, subdirs, flows[0], fr.fparams(**kw))
    assert got[0].tobytes() == want.tobytes(), (got[0], want)
    return got[0]


def grid64(aof):
    X, Y = fr.coordinates(p64(aof))
    assert X.size == 49 and sorted(set(X.tolist())) == [16 * b - 48 for b in range(7)] and (X.reshape(7, 7)[0] == Y.reshape(7, 7)[:, 0]).all()
    return X, Y


# ---- hand literals -----------------------------------------------------------------------------------------------------
def test_a_pure_shift_has_no_zoom_and_no_rotation_and_its_centre_is_the_shift(aof):
    X, _ = grid64(aof)
    b, sd = fr.records_of(np.full(49, 4), np.full(49, -3), 100)       # 2 px right, 1.5 px up
    f = both(aof, p64(aof), b, sd)
    assert (f["zoom"], f["rotation"], f["centre_x"], f["centre_y"]) == (0.0, 0.0, 2.0, -1.5)
    assert (f["accepted"], f["at_reach"], f["fitted"], f["used"], f["flags"]) == (49, 0, 49, 49, fr.VALID | fr.REFIT)
    assert f["num_zoom"] == 0 and f["num_rot"] == 0 and f["det"] == 49 * int((X * X).sum()) * 2 and f["reserved"] == 0


@pytest.mark.parametrize("zoom, rot", [(1, 0), (0, 1), (1, 1), (-1, 1)])
def test_a_sixteenth_of_zoom_and_rotation_comes_back_exactly(aof, zoom, rot):
    X, Y = grid64(aof)
    U, V = 1 + (zoom * X - rot * Y) // 16, (rot * X + zoom * Y) // 16       # whole half-pixels: X and Y are multiples of 16; |dx|, |dy| <= 3
    b, sd = fr.records_of(U, V, 0)
    f = both(aof, p64(aof), b, sd)
    assert (f["zoom"], f["rotation"]) == (zoom * 0.0625, rot * 0.0625)
    assert (f["centre_x"], f["centre_y"]) == (0.5, 0.0) and f["used"] == 49
    assert f["det"] * zoom == 16 * f["num_zoom"] and f["det"] * rot == 16 * f["num_rot"]


# ---- outliers ----------------------------------------------------------------------------------------------------------
def test_the_second_pass_drops_five_wild_blocks_of_49(aof):
    X, Y = grid64(aof)
    U, V = X // 16, Y // 16
    wild = [16, 18, 24, 30, 32]
    U[wild], V[wild] = U[wild] + 5, V[wild] - 5                              # 2.5 px off, none at the reach
    b, sd = fr.records_of(U, V, 0)
    f = both(aof, p64(aof), b, sd)
    assert (f["zoom"], f["rotation"], f["centre_x"], f["centre_y"]) == (0.0625, 0.0, 0.0, 0.0)
    assert (f["fitted"], f["used"], f["flags"]) == (49, 44, fr.VALID | fr.REFIT)
    one = both(aof, p64(aof), b, sd, passes=1)
    assert (one["fitted"], one["used"], one["flags"]) == (49, 49, fr.VALID)
    assert one["centre_x"] != 0.0 and abs(one["centre_x"] - 0.5 * 25 / 49) < 1e-6      # the mean of the wild shifts leaks into it


# ---- degenerate inputs ---------------------------------------------------------------------------------------------------
def zero_but(accepted=0, at_reach=0):
    z = np.zeros((), fr.FIELD_DTYPE)
    z["accepted"], z["at_reach"] = accepted, at_reach
    return z


def test_all_blocks_skipped(aof):
    b, sd = fr.records_of(np.full(49, 2), np.full(49, 2), fr.SKIPPED)
    assert both(aof, p64(aof), b, sd).tobytes() == zero_but().tobytes()


def test_fewer_blocks_than_min_blocks(aof):
    X, Y = grid64(aof)
    sad = np.full(49, fr.SKIPPED)
    sad[[0, 6, 24, 42, 48, 3, 21]] = 0
    b, sd = fr.records_of(X // 16, Y // 16, sad)
    assert both(aof, p64(aof), b, sd).tobytes() == zero_but(7).tobytes()
    f = both(aof, p64(aof), b, sd, min_blocks=7)
    assert (f["zoom"], f["used"], f["flags"]) == (0.0625, 7, fr.VALID | fr.REFIT)
    row = np.full(49, fr.SKIPPED)
    row[:3] = 0                                                             # three blocks of ONE row: Y is constant, D > 0 through X alone
    b, sd = fr.records_of(X // 16, Y // 16, row)
    f = both(aof, p64(aof), b, sd, min_blocks=3)
    assert f["flags"] == fr.VALID | fr.REFIT and f["det"] == 3 * (48 * 48 + 32 * 32 + 16 * 16) - 96 * 96 and f["zoom"] == 0.0625


def test_every_block_at_reach(aof):
    b, sd = fr.records_of(np.full(49, 8), np.full(49, 0), 0)                 # dx == S everywhere
    assert both(aof, p64(aof), b, sd).tobytes() == zero_but(49, 49).tobytes()
    f = both(aof, p64(aof), b, sd, exclude_reach=0)
    assert (f["at_reach"], f["used"], f["centre_x"], f["zoom"]) == (49, 49, 4.0, 0.0)


def test_a_second_set_below_min_blocks_publishes_the_first(aof):
    X, _ = grid64(aof)
    U = np.where((np.arange(49) % 2) == 0, 5, -5)                            # a checkerboard of +-2.5 px: nobody within 1 px of the fit
    b, sd = fr.records_of(U, -U, 0)
    f = both(aof, p64(aof), b, sd)
    assert (f["fitted"], f["used"], f["flags"]) == (49, 49, fr.VALID)
    assert abs(f["centre_x"] - 0.5 * 5 / 49) < 1e-6


# ---- edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value_threshold", [3000, 0x20000, 1, 0])
def test_the_acceptance_rule_is_reduces(aof, orc, value_threshold):
    p = p64(aof, value_threshold=value_threshold)
    T = vf.threshold_of(p)
    sads = np.array([max(T - 1, 0), T, 0xFFFE, 0xFFFF])
    X, Y = grid64(aof)
    b, sd = fr.records_of(X // 16, Y // 16, sads[np.arange(49) % 4])
    f = both(aof, p, b, sd, min_blocks=3)
    want = int(((b["sad"] != 0xFFFF) & (b["sad"] < T)).sum())
    assert f["accepted"] == want
    assert orc.reduce(orc.params_from(p), b, sd, vf.level_range(p))[0]["count"] == want      # accepted == aof_flow.count


def test_two_levels_measure_the_reach_from_the_predictor(aof):
    p = p64(aof, pyramid_levels=2)
    dx = np.array([6, -2, 4, 2, 0, -1, 3] * 7)                                # predictor (2, -1): 6 and -2 sit at the reach, 4 does not
    b = np.zeros(49, fr.BLOCK_DTYPE)
    b["dx"], b["dy"] = dx, -1
    f = both(aof, p, b, None, flows_of(1, (2, -1)))
    assert (f["accepted"], f["at_reach"], f["fitted"]) == (49, 14, 35)
    b["dy"] = 3                                                               # |3 - (-1)| == S: every block at reach through y
    assert both(aof, p, b, None, flows_of(1, (2, -1)))["at_reach"] == 49
    assert both(aof, p, b, None, flows_of(1, (0, 0)))["at_reach"] == 7        # (dx == 4 alone)


def test_no_subdirs_is_all_eights(aof):
    b, sd = fr.d_random(p64(aof), np.random.default_rng(5))
    b["sad"] = 0
    assert both(aof, p64(aof), b, None).tobytes() == both(aof, p64(aof), b, np.full(49, 8, np.uint8)).tobytes()
    assert both(aof, p64(aof), b, None).tobytes() != both(aof, p64(aof), b, sd).tobytes()


# ---- the host function against the model, every geometry -----------------------------------------------------------------
@pytest.mark.parametrize("geom", fr.GEOMETRIES, ids=[g[0] for g in fr.GEOMETRIES])
def test_host_equals_model(aof, geom):
    p = fr.make_params(aof, geom)
    g = vf.grid_of(p, 0)
    assert g.nx * g.ny == fr.NBLOCKS[geom[0]] and tuple(aof.grid(p, 0)) == tuple(g) and aof.field_supported(p)
    recs = [vf.records_of_design(p, vf.design("uniform-random", g.ny, g.nx, vf.level_range(p), variant, half=bool(p.subpixel))) for variant in range(2)]
    blocks = np.stack([r[0] for r in recs])
    subdirs = np.stack([r[1] for r in recs]) if p.subpixel else None
    flows = flows_of(2, (0, 0))
    for kw in (dict(), dict(passes=1), dict(exclude_reach=0, gate_px=0.5), dict(min_blocks=3, gate_px=3.0)):
        got = aof.field_host(p, blocks, flows, subdirs, aof.field_params(**kw))
        assert got.tobytes() == fr.model_batch(p, blocks, subdirs, flows, fr.fparams(**kw)).tobytes(), kw
    blocks, subdirs, flows = fr.batch(p, 6, seed=1)
    for sub in (subdirs, None):
        for kw in (dict(), dict(passes=1, exclude_reach=0)):
            got = aof.field_host(p, blocks, flows, sub, aof.field_params(**kw))
            want = fr.model_batch(p, blocks, sub, flows, fr.fparams(**kw))
            assert got.tobytes() == want.tobytes(), (kw, sub is None, got, want)
    assert (got["flags"] & fr.VALID).any() and not (got["flags"] & fr.VALID).all()


@pytest.mark.parametrize("geom", [fr.LARGEST, fr.LARGEST_ODD], ids=lambda g: g[0])
def test_conversions_beyond_2_to_53_round_to_nearest_on_the_host(aof, geom):
    p = fr.make_params(aof, geom)
    assert aof.field_supported(p) and vf.grid_of(p).nx * vf.grid_of(p).ny == int(geom[0].split("-")[1])
    blocks, subdirs, flows = fr.batch(p, 2, seed=3, designs=("extreme", "similarity"))
    for kw in (dict(exclude_reach=0), dict(exclude_reach=0, passes=1)):      # (the gate of two passes keeps few of the extreme blocks)
        got = aof.field_host(p, blocks, flows, subdirs, aof.field_params(**kw))
        assert got.tobytes() == fr.model_batch(p, blocks, subdirs, flows, fr.fparams(**kw)).tobytes()
    assert (np.abs(got["det"]) > 2 ** 53).all() and abs(int(got["num_zoom"][0])) > 2 ** 53 and (got["flags"] & fr.VALID).all()
    if geom is fr.LARGEST_ODD:
        inexact = lambda v: float(int(v)) != int(v)
        assert inexact(got["det"][0]) and inexact(got["num_zoom"][0]) and inexact(got["det"][1]), "no operand of this case needs rounding"


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_defaults_and_exports(aof):
    assert C.sizeof(aof.FieldParams) == 16 and aof.FIELD_DTYPE.itemsize == 64 and aof.FIELD_DTYPE == fr.FIELD_DTYPE
    fp = aof.field_params()
    assert (fp.min_blocks, fp.passes, fp.exclude_reach, fp.gate_px) == (8, 2, 1, 1.0)
    for name in ("aof_field_params_default", "aof_field_supported", "aof_field_batch_device", "aof_field_host"):
        assert name in aof.EXPORTS and getattr(aof.lib, name).restype is C.c_int
    assert aof.lib.aof_field_params_default(None) == -22
    assert (aof.FIELD_VALID, aof.FIELD_REFIT) == (fr.VALID, fr.REFIT)


def test_refusals_of_the_host_function(aof):
    p = p64(aof)
    b, f, out = np.zeros((1, 49), fr.BLOCK_DTYPE), flows_of(1), np.full(1, 7, dtype=fr.FIELD_DTYPE)
    call = lambda p_, fp, bl, fl, n, o: aof.lib.aof_field_host(p_, fp, bl, None, fl, n, o)
    ok = aof.field_params()
    args = [C.byref(p), C.byref(ok), b.ctypes.data, f.ctypes.data, 1, out.ctypes.data]
    assert call(*args) == 0
    before = out.tobytes()
    for i in (0, 1, 2, 3, 5):
        bad = list(args)
        bad[i] = None
        assert call(*bad) == -22
    assert call(*args[:4], -1, args[5]) == -22
    for kw in (dict(min_blocks=2), dict(passes=0), dict(passes=3), dict(exclude_reach=2), dict(exclude_reach=-1), dict(gate_px=0.0),
               dict(gate_px=-1.0), dict(gate_px=float("inf")), dict(gate_px=float("nan"))):
        assert call(args[0], C.byref(aof.field_params(**kw)), *args[2:]) == -22, kw
    assert call(C.byref(p64(aof, tile=12)), *args[1:]) == -22
    assert out.tobytes() == before
    assert call(args[0], C.byref(aof.field_params(min_blocks=3, gate_px=1e-30)), *args[2:]) == 0


def test_supported_at_both_sides_of_its_bound(aof):
    inside, outside = aof.default_params(4096, 4096), aof.default_params(8192, 2048)
    assert aof.check_params(inside) == 0 and aof.check_params(outside) == 0
    assert fr.range_product(inside) < 2 ** 62 <= fr.range_product(outside)
    assert aof.field_supported(inside) and not aof.field_supported(outside)
    assert aof.lib.aof_field_supported(C.byref(outside)) == -22 and aof.lib.aof_field_supported(None) == -22
    assert not aof.field_supported(aof.default_params(64, 64, tile=12))
    # closer: the same 8192 x 2048 frame on 16 x 16 tiles has a quarter of the blocks
    near = aof.default_params(8192, 2048, tile=16, search=8)
    assert fr.range_product(near) < 2 ** 62 and aof.field_supported(near)
    # the largest sparse grids the bound admits and the first it refuses, by the grid's density
    for nbk in range(100, 2000, 100):
        p = aof.px4flow_params(4096, 4096, num_blocks=nbk)
        assert aof.field_supported(p) == (fr.range_product(p) < 2 ** 62), nbk
    b, f = np.zeros((1, vf.grid_of(outside).nx * vf.grid_of(outside).ny), fr.BLOCK_DTYPE), flows_of(1)
    with pytest.raises(aof.AofError):
        aof.field_host(outside, b, f)


# ---- accuracy: what the fit is for ---------------------------------------------------------------------------------------
CONFIGS = {
    "dense128": lambda aof: aof.default_params(128, 128),
    "px4flow128": lambda aof: aof.px4flow_params(128, 128),
    "c5": lambda aof: aof.default_params(1280, 960, tile=16, search=8, value_threshold=12000),
}
# Worst errors over the five WARP_PRESETS at noise 0 and 4 LSB (seeded inputs, a deterministic oracle), measured with the
# rule as it stands and rounded up to the next 0.01 px / 0.001 (LAB_LOG.md, "Motion field"): (centre px, zoom, rotation rad)
BOUNDS = {"dense128": (0.02, 0.003, 0.003), "px4flow128": (0.09, 0.006, 0.003), "c5": (1.27, 0.007, 0.032)}


@functools.lru_cache(maxsize=None)
def _measured(config):
    import __graft_entry__ as ge
    import importlib
    from oracle import pyoracle as orc
    aof = ge.load_package()
    synth = importlib.import_module("aero_optical_flow_amd.synth")
    p = CONFIGS[config](aof)
    rows = []
    for k, preset in enumerate(sorted(synth.WARP_PRESETS)):
        for noise in (0, 4):
            prev, cur, truth = synth.make_warp_pair(p.width, p.height, reach=2, pair_index=k, noise=noise, preset=preset)
            ref = orc.flow_pair(orc.params_from(p), prev, cur)
            sub = ref["subdirs"] if p.subpixel else None
            f = fr.model(p, ref["blocks"], sub, ref["flow"])
            assert f["flags"] & fr.VALID and f["accepted"] == ref["flow"]["count"]
            assert aof.field_host(p, ref["blocks"][None], ref["flow"].reshape(1), None if sub is None else sub[None])[0].tobytes() == f.tobytes()
            a = synth.WARP_PRESETS[preset]
            inv = np.linalg.inv(np.array([[a[0], a[1]], [a[2], a[3]]], np.float64) / 65536.0)
            h, w = p.height // 2, p.width // 2
            centre = truth[h - 1:h + 1, w - 1:w + 1].astype(np.float64).mean(axis=(0, 1))      # the frame centre lies between four pixels
            rows.append(dict(preset=preset, noise=noise,
                             centre=max(abs(f["centre_x"] - centre[0]), abs(f["centre_y"] - centre[1])),
                             hist=max(abs(ref["flow"]["flow_x"] - centre[0]), abs(ref["flow"]["flow_y"] - centre[1])),
                             zoom=abs(f["zoom"] - (inv[0, 0] - 1.0)), rotation=abs(f["rotation"] - inv[1, 0]),
                             used=int(f["used"]), at_reach=int(f["at_reach"])))
    return rows


@pytest.mark.parametrize("config", list(CONFIGS))
def test_the_fit_recovers_centre_flow_zoom_and_rotation(config):
    rows = _measured(config)
    worst = {k: max(r[k] for r in rows) for k in ("centre", "zoom", "rotation", "hist")}
    print(f"\n{config}: worst centre {worst['centre']:.4f} px, zoom {worst['zoom']:.5f}, rotation {worst['rotation']:.5f} rad; histogram flow {worst['hist']:.3f} px")
    for r in rows:
        print("   ", {k: (round(float(v), 5) if not isinstance(v, (str, int)) else v) for k, v in r.items()})
    centre, zoom, rotation = BOUNDS[config]
    assert worst["centre"] <= centre and worst["zoom"] <= zoom and worst["rotation"] <= rotation, worst


def test_the_histogram_flow_misses_a_rotation_that_the_fit_finds():
    row = next(r for r in _measured("dense128") if r["preset"] == "rotate_2" and r["noise"] == 0)
    assert row["hist"] > 0.5 and row["centre"] <= BOUNDS["dense128"][0], row
