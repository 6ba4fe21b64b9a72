"""CPU: vtmhip_smvd_launch_form, the launch rule of vtmhip_smvd_batch_dev as host arithmetic (no context: a device of 256 compute units)."""
import ctypes as C

import me_util
from vtm_amd import lib

GEN64, GEN256, GROUP, WORKGROUP = 0, 1, 2, 3      # VTMHIP_SMVD_KERNEL_*
OK = lib.OK


def form(w, h, bd, uniform, n):
    out = [C.c_int(-1) for _ in range(4)]
    st = lib.load().vtmhip_smvd_launch_form(None, w, h, bd, int(uniform), n, *[C.byref(v) for v in out])
    return st, tuple(v.value for v in out)


def test_tile_shapes_and_their_forms():
    """the 17 shapes of the tile kernel: the group form up to eight 8x8 tiles (eight slots up to eight waves per compute unit, four above), one wave per PU at 16
    tiles, four above; everything else, 12 bits and mixed batches take the general kernel by the hint's area"""
    shapes = [(w, h) for w in range(4, 129, 4) for h in range(4, 129, 4)]
    tiled = [s for s in shapes if form(s[0], s[1], 10, True, 100)[1][0] in (GROUP, WORKGROUP)]
    assert sorted(tiled) == sorted(me_util.SMVD_TILE_SHAPES)
    for w, h in shapes:
        general = (OK, (GEN64 if w * h <= 1024 else GEN256, 0, 0, 0))
        assert form(w, h, 12, True, 100) == general and form(w, h, 10, False, 100) == general
        if (w, h) not in tiled:
            assert form(w, h, 10, True, 100) == form(w, h, 8, True, 100) == general
    for w, h in me_util.SMVD_TILE_SHAPES:
        t = (w // 8) * (h // 8)
        for bd in (8, 9, 10):
            if t <= 8:
                thr = 8 * 256 * (64 // (8 * t))      # 16 384 / 8 192 / 4 096 / 2 048 jobs
                for n in (0, 1, thr):
                    assert form(w, h, bd, True, n) == (OK, (GROUP, 0, 8, 64 // (8 * t))), (w, h, n)
                for n in (thr + 1, 172500, 2 ** 31 - 1):
                    assert form(w, h, bd, True, n) == (OK, (GROUP, 0, 4, 64 // (4 * t))), (w, h, n)
            else:
                for n in (1, 5000, 2 ** 31 - 1):
                    assert form(w, h, bd, True, n) == (OK, (WORKGROUP, 1 if t == 16 else 4, 8, 1)), (w, h, n)


def test_arguments_and_the_switch(monkeypatch):
    for w, h, bd, n in ((0, 8, 10, 1), (8, 132, 10, 1), (6, 8, 10, 1), (8, 8, 7, 1), (8, 8, 13, 1), (8, 8, 10, -1)):
        assert form(w, h, bd, True, n) == (lib.E_INVALID, (-1, -1, -1, -1))
    assert lib.load().vtmhip_smvd_launch_form(None, 8, 8, 10, 1, 1, None, None, None, None) == lib.E_INVALID
    monkeypatch.setenv("VTMHIP_SMVD_NO_TILE", "1")      # the environment switch of the entry: the general kernel for everything
    assert form(8, 8, 10, True, 100) == (OK, (GEN64, 0, 0, 0)) and form(64, 64, 10, True, 100) == (OK, (GEN256, 0, 0, 0))
    monkeypatch.delenv("VTMHIP_SMVD_NO_TILE")
    assert form(8, 8, 10, True, 100)[1][0] == GROUP
