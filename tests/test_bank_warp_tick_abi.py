"""The host side of the one-launch tick with the warp inside it (include/aof.h, "the stream bank with a lens"), without a
GPU: aof_bank_last_path's refusals, and aof_bank_warp_one_launch against the LDS arithmetic of tests/small_plan_ref.py
(small_plan_make's model) plus the mesh's 8 nx ny bytes of nodes.

The LDS border: on the published sparse grid (px4flow_params: 25 .. 36 blocks whatever the frame size) the one-workgroup
class accepts frames up to the LDS limit, so width / height pairs on each side of the border exist; they are searched with
the model here, and the test holds the library to the byte on both sides -- at a border where the nodes alone decide (the
plain plan of the frame beyond it still fits) wherever the search finds one, which it does."""
import ctypes as C

import bank_warp_ref as wref
import small_plan_ref as sp

EINVAL = -22


def model(w, h, levels):
    """(dynamic LDS bytes of the warped tick, does it fit): small_plan_make's bytes, the nodes behind them."""
    nx, ny = wref.mesh_size(w, h)
    lds = sp.small_lds(w, h, levels) + 8 * nx * ny
    return lds, lds + sp.STATIC_LDS <= sp.LDS_LIMIT


def px4_plan_ok(w, h):
    """The one-workgroup class on the sparse grid of a one-level w x h frame: the grouped search (8 .. 256 blocks) and
    small_plan_make's verdict."""
    g = sp.grid_for_level(w, h, 0, True, 1)
    if not 8 <= sp.blocks(g) <= sp.THREADS:
        return False
    return sp.small_plan(w, h, 1, g, None, 1, w * h, sp.BASE, sp.BASE, 1)["verdict"] == "ok"


def test_last_path_refuses_null(aof):
    assert aof.lib.aof_bank_last_path(None) == EINVAL


def test_a_fresh_context_has_made_no_push(aof):
    """0 before the first push (where this machine has a device to create a context on; the GPU tests ask again)."""
    ctx = C.c_void_p()
    p = aof.px4flow_params(64, 64)
    if aof.lib.aof_create(C.byref(p), 0, C.byref(ctx)) == 0:
        assert aof.lib.aof_bank_last_path(ctx) == 0
        aof.lib.aof_destroy(ctx)
    assert callable(aof.FlowEngine.last_bank_path) and callable(aof.OpticalFlowBank.lastPushPath)


def test_one_launch_refuses_null(aof):
    lds = C.c_int64(-1)
    assert aof.lib.aof_bank_warp_one_launch(None, C.byref(lds)) == EINVAL and lds.value == -1
    assert aof.lib.aof_bank_warp_one_launch(C.byref(aof.px4flow_params(64, 64)), None) == 1, "the byte count is optional"


def test_the_two_flagship_configurations_run_in_one_launch(aof):
    ok, lds = aof.bank_warp_one_launch(aof.px4flow_params(64, 64))
    assert (ok, lds) == (True, model(64, 64, 1)[0]) and lds == 2 * (64 * 64 + 16) + 648
    ok, lds = aof.bank_warp_one_launch(aof.px4flow_params(128, 128, pyramid_levels=2, mean_subtract=1))
    assert (ok, lds) == (True, model(128, 128, 2)[0]) and lds == 2 * (128 * 128 + 16) + 2 * (64 * 64 + 16) + 2312
    assert sp.small_lds(64, 64, 1) % 16 == 0 and sp.small_lds(128, 128, 2) % 16 == 0, "the node region starts on 16 bytes"


def test_a_configuration_the_plan_refuses_returns_zero(aof):
    dense = aof.default_params(640, 480)               # a dense grid of thousands of blocks: the separate kernels
    assert aof.bank_warp_one_launch(dense)[0] is False
    narrow = aof.px4flow_params(72, 64)                # a width that is no multiple of 16
    assert aof.check_params(narrow) == 0 and aof.bank_warp_one_launch(narrow)[0] is False
    bad = aof.px4flow_params(64, 64)
    bad.tile = 7
    assert aof.check_params(bad) != 0 and aof.bank_warp_one_launch(bad)[0] is False


def border_pairs():
    """[(w, h)] accepted by the class with (w, h + 1) beyond the LDS border; first those where the nodes alone decide."""
    found = []
    for w in range(64, 513, 16):
        h = 64
        while px4_plan_ok(w, h + 1) and model(w, h + 1, 1)[1]:
            h += 1
        if px4_plan_ok(w, h) and model(w, h, 1)[1] and not model(w, h + 1, 1)[1]:
            nodes_decide = sp.small_lds(w, h + 1, 1) + sp.STATIC_LDS <= sp.LDS_LIMIT
            found.append((not nodes_decide, w, h))
    return [(w, h) for _, w, h in sorted(found)]


def test_the_lds_border_to_the_byte(aof):
    pairs = border_pairs()
    assert pairs, "the model finds width / height pairs on each side of the border"
    w0, h0 = pairs[0]
    assert sp.small_lds(w0, h0 + 1, 1) + sp.STATIC_LDS <= sp.LDS_LIMIT, "a border at which the nodes alone decide"
    for w, h in pairs[:6]:
        under, over = aof.px4flow_params(w, h), aof.px4flow_params(w, h + 1)
        assert aof.check_params(under) == 0 and aof.check_params(over) == 0, (w, h)
        assert aof.bank_warp_one_launch(under) == (True, model(w, h, 1)[0]), (w, h)
        assert aof.bank_warp_one_launch(over) == (False, model(w, h + 1, 1)[0]), (w, h + 1)
        slack = sp.LDS_LIMIT - sp.STATIC_LDS - model(w, h, 1)[0]
        assert 0 <= slack < 2 * w + 8 * wref.mesh_size(w, h)[0], ("one more row would not fit", w, h, slack)


def test_the_crossover_query(aof):
    assert 0 <= aof.bank_warp_crossover() <= 4096
