"""The host model of the 16x16 probe (tile16_probe_ref.py) against hand answers and brute force (CPU).  The GPU side holds
k_tile16_probe to this model word for word (test_gpu_tile16_verdicts.py)."""
import numpy as np
import pytest

import npref
import tile16_probe_ref as ref


def dense16(w, h, **kw):
    p = dict(width=w, height=h, tile=16, search=8, grid_mode=0, subpixel=0, mean_subtract=0, num_blocks=0)
    p.update(kw)
    return p


def texture(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def test_identical_random_frames_separate_on_one_row():
    img = texture(256, 320, 1)
    assert ref.level0_word(dense16(320, 256), img, img) == 2          # separation 0: every best row's bound is 0


def test_flat_frames_go_to_the_exhaustive_scan():
    flat = np.full((256, 320), 90, np.uint8)
    for kw in (dict(), dict(subpixel=1), dict(mean_subtract=1)):
        assert ref.level0_word(dense16(320, 256, **kw), flat, flat) == 0, kw


def test_a_predictor_that_moves_every_sample_window_out_of_the_frame():
    img = texture(256, 320, 2)
    p = dense16(320, 256)
    for pred in ((400, 0), (0, -300), (-200, 0), (0, 250)):
        assert ref.level0_word(p, img, img, pred) == 1, pred           # nothing sampled: "pruning pays", separation 0
    assert ref.level0_word(p, img, img, (3, -2)) != 1


@pytest.mark.parametrize("kw", [dict(), dict(subpixel=1)])
def test_two_row_bounds_against_brute_force_sads(kw):
    """Bound of (block, dy) = the smallest over dx of the SAD of tile rows 4 and 12 alone, summed by npref.sad on those two
    rows of the tile and of the window; the full SAD of a row against npref.sad of the whole tile."""
    rng = np.random.default_rng(7)
    prev = texture(256, 320, 3)
    cur = np.clip(np.roll(prev, (2, -3), axis=(0, 1)).astype(np.int64) + rng.integers(-9, 10, prev.shape), 0, 255).astype(np.uint8)
    p = dense16(320, 256, **kw)
    x0 = 9 if kw.get("subpixel") else 8
    delta, pred = -5, (2, 1)
    ceq = npref.equalise(cur, delta)
    for bx, by, dy in ((0, 0, 0), (4, 3, 8), (11, 7, 16), (17, 13, 5)):
        rs = ref.row_sads(prev, cur, x0, bx, by, pred, delta)
        tx, ty = x0 + 16 * bx, x0 + 16 * by                            # tile origin in the frame
        wy = ty - 8 + pred[1] + dy                                     # window row of candidate row dy
        rows = [4, 12]
        want = min(npref.sad(prev[[ty + r for r in rows]], tx, 0, ceq[[wy + r for r in rows]], tx - 8 + pred[0] + dx, 0, 16)
                   for dx in range(17))
        assert int(ref.bounds(rs, ref.TWO_ROWS)[dy]) == want, (bx, by, dy)
        assert ref.full_sad(rs, dy) == min(npref.sad(prev, tx, ty, ceq, tx - 8 + pred[0] + dx, wy, 16) for dx in range(17))
    assert ref.level0_word(p, prev, cur) == ref.probe_word(prev, cur, x0, (320 - 2 * x0) // 16, (256 - 2 * x0) // 16)


@pytest.mark.parametrize("size", [(32, 5008), (48, 2000), (64, 64), (480, 48)])
def test_sample_grids_of_narrow_tall_and_tiny_frames(size):
    w, h = size
    nx, ny = (w - 16) // 16, (h - 16) // 16
    blocks = ref.sample_blocks(nx, ny)
    assert 1 <= len(blocks) <= ref.K_PROBE_MAX_BLOCKS
    assert len(set(blocks)) == len(blocks)
    assert all(0 <= bx < nx and 0 <= by < ny for bx, by in blocks), (nx, ny, blocks)
    stx, sty = ref.sample_strides(nx, ny)
    assert ref.probe_samples(nx, stx) >= 1 and ref.probe_samples(ny, sty) >= 1


def test_sample_grid_of_a_vga_like_frame():
    # 79 x 59 blocks (1280 x 960): every eighth block per axis from the fourth, 10 x 7 of them
    blocks = ref.sample_blocks(79, 59)
    assert ref.sample_strides(79, 59) == (8, 8) and len(blocks) == 70
    assert blocks[0] == (4, 4) and blocks[9] == (76, 4) and blocks[-1] == (76, 52)
    # 2 000 x 10 blocks: 250 x 1 samples, the x stride doubles until 128 blocks fit; 100 x 100: 12 x 12, a tie goes to x
    assert ref.sample_strides(2000, 10) == (16, 8) and len(ref.sample_blocks(2000, 10)) == 125
    assert ref.sample_strides(100, 100) == (16, 8) and len(ref.sample_blocks(100, 100)) == 72
