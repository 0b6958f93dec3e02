"""GPU ORB extraction against the independent NumPy restatement (tests/orb_ref_py.py), stage by
stage through all seven debug buffers, at the tiling edges of the six kernels.

Every comparison is exact.  Each shape of the table below is there for a reason, and the reason
is asserted on the CPU inside the test from the restated level and cell geometry
(ORBextractor.cc:769-806, :1115-1116), so the coverage is checked and not supposed.

Debug buffers (OrbEngine::debug_fetch) and how they are decoded here:
  0  pyramid, 1 blurred pyramid: the levels back to back, each w x h bytes, rows packed.
  2  int32 per FAST cell: keys k_fast left in the cell.  Cells are numbered level-major, inside a
     level in the order of the reference's loop (rows, then columns; skipped cells get no number).
  3  uint32 key slots.  Cell c owns slots [off_c, off_c + cap_c) with cap_c = ceil(R/2) *
     ceil(C/2) for its R x C detection window (the most strict-NMS survivors it can hold) and
     off_c the running sum.  k_fast packs a key as  y << 20 | x << 8 | score  with (x, y)
     relative to the level's minBorder corner (16, 16) -- the frame of the reference's
     vToDistributeKeys.  The order of the keys inside a cell is the kernel's own: sets compared.
  4  uint32 octree output keys, level l at [out_off_l, out_off_l + max(N_l, 4 nIni_l) + 8), same
     packing with (x, y) in level coordinates (minBorder added, ORBextractor.cc:843-844).  The
     slot count follows DistributeOctTree's bound: at most N + 2 keys once a pass starts below
     N, but the first pass makes up to 4 nIni nodes of the nIni initial ones whatever N is.
  5  int32 per level: keys the octree kept.
  6  int32 device error flags.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import multimot_track_amd as M
import orb_ref_py as R
from multimot_track_amd import synthetic

pytestmark = pytest.mark.gpu

NF = 300  # features per frame wherever the shape is the point


# ------------------------------------------------------------------ restated geometry
def _levels(w, h):
    return R.level_sizes(w, h)


def _accepted(w, h):
    """Every level has at least one 30-px FAST cell row and column (else :784-787 divide by 0)."""
    return all(lw - 32 >= 30 and lh - 32 >= 30 for lw, lh in _levels(w, h))


def _cells(w, h):
    return [R.level_cells(lw, lh) for lw, lh in _levels(w, h)]


def _fast_tile(w, h):
    """LDS tile width of the widest cell, ((cols + 4) & ~3): <= 40 runs k_fast<40>, else <72>."""
    return max((c[5] - c[4] + 4) & ~3 for lv in _cells(w, h) for c in lv)


def _widest_cell(w, h):
    return max(c[5] - c[4] for lv in _cells(w, h) for c in lv)


def _n_ini(w, h):
    return [R.n_ini(16, lw - 16, 16, lh - 16) for lw, lh in _levels(w, h)]


def _lw(w, h):
    return [a for a, _ in _levels(w, h)]


def _lh(w, h):
    return [b for _, b in _levels(w, h)]


WMIN, HMIN = 221, 221

# name -> (w, h, why): `why` must hold for the shape to be in the table.  The shapes are the
# smallest (width first, at the smallest accepted height, or the reverse) that a search over
# 221..700 (1229..1260 for the two wide ones) found for each condition.
SHAPES = {
    # smallest accepted image: level 7 is 62 x 62 with exactly one FAST cell; nIni = 1 on every
    # level; its level 2 is 153 rows, one row more than a multiple of the 8-row k_resize band
    "smallest": (WMIN, HMIN, lambda w, h: (
        _accepted(w, h) and not _accepted(w - 1, h) and not _accepted(w, h - 1) and
        _levels(w, h)[7] == (62, 62) and len(_cells(w, h)[7]) == 1 and
        set(_n_ini(w, h)) == {1} and any(v % 8 == 1 for v in _lh(w, h)[1:]))),
    # every cell at most 36 px wide: tile <= 40, the k_fast<40> instantiation; nIni = 2
    "fast40": (453, HMIN, lambda w, h: _fast_tile(w, h) <= 40 and min(_n_ini(w, h)) >= 2),
    # a level 91 px wide: one cell column of 59 px, the widest cell the geometry allows (tile
    # 60; tests/test_orb_ref_py.py::test_fast_tile_geometry_bound), k_fast<72>
    "cell59": (226, HMIN, lambda w, h: (
        _widest_cell(w, h) == 59 and _fast_tile(w, h) == 60 and 91 in _lw(w, h))),
    # last k_blur tile (256 columns) 1, 2, 3 columns wide: at level 0 ...
    "blur_w1_l0": (257, HMIN, lambda w, h: w % 256 == 1),
    "blur_w2_l0": (258, HMIN, lambda w, h: w % 256 == 2),
    "blur_w3_l0": (259, HMIN, lambda w, h: w % 256 == 3),
    # ... and at level 1
    "blur_w1_l1": (308, HMIN, lambda w, h: _lw(w, h)[1] % 256 == 1),
    "blur_w2_l1": (309, HMIN, lambda w, h: _lw(w, h)[1] % 256 == 2),
    "blur_w3_l1": (311, HMIN, lambda w, h: _lw(w, h)[1] % 256 == 3),
    # a level (3: 129 rows) whose last 32-row k_blur band is one row
    "blur_h1": (WMIN, 223, lambda w, h: _lh(w, h)[3] % 32 == 1),
    # level 1 exactly 1024 wide (one full k_resize column block) and 1025 (a second block of one
    # column); both run k_fast<40>
    "resize_1024": (1229, HMIN, lambda w, h: _lw(w, h)[1] == 1024 and _fast_tile(w, h) <= 40),
    "resize_1025": (1230, HMIN, lambda w, h: _lw(w, h)[1] == 1025 and _fast_tile(w, h) <= 40),
    # the shape the older tests use: nIni = 2 on every level, k_fast<72> (tile 48)
    "400x260": (400, 260, lambda w, h: set(_n_ini(w, h)) == {2} and 40 < _fast_tile(w, h) <= 72),
}


def _slot_layout(w, h):
    """Per level: [(slot offset, slot capacity)] per cell, and the level's first cell number."""
    off, ncell, out = 0, 0, []
    for lv in _cells(w, h):
        lay = []
        for (_, _, r0, r1, c0, c1, _, _) in lv:
            rr, cc = max(r1 - r0 - 6, 0), max(c1 - c0 - 6, 0)
            cap = ((rr + 1) // 2) * ((cc + 1) // 2)
            lay.append((off, cap))
            off += cap
        out.append((ncell, lay))
        ncell += len(lv)
    return out, ncell, off


def _unpack(keys):
    keys = np.asarray(keys, np.uint32)
    return np.stack([(keys >> 8) & 0xFFF, keys >> 20, keys & 0xFF], 1).astype(np.int64)


def _split_levels(flat, w, h):
    out, off = [], 0
    for lw, lh in _levels(w, h):
        out.append(flat[off:off + lw * lh].reshape(lh, lw))
        off += lw * lh
    assert off == len(flat), "pyramid buffer holds %d bytes, levels sum to %d" % (len(flat), off)
    return out


@functools.lru_cache(maxsize=None)
def _frame(w, h, seed):
    g = synthetic.gray_frame(h, w, seed)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _ref(w, h, seed, nf):
    """The restatement's stages for one synthetic frame, computed once per module."""
    return R.orb_stages(_frame(w, h, seed), nf)


def _ctx(w, h, nf=NF, batch=1):
    return M.Context(M.kitti03_config(w, h, nf, max_batch=batch))


def _check_buffers(ctx, st, w, h, tag, frame=0, keys=True):
    """Buffers 0-6 of `frame` against the restatement's stages `st`."""
    lv = ctx.levels()
    assert list(zip(lv["level_w"].tolist(), lv["level_h"].tolist())) == _levels(w, h)
    assert lv["n_per_level"].tolist() == st["cfg"]["n_per_level"]
    R.check_images(tag + " pyramid (buffer 0)", _split_levels(ctx.debug_fetch(0, frame), w, h),
                   st["pyramid"])
    R.check_images(tag + " blur (buffer 1)", _split_levels(ctx.debug_fetch(1, frame), w, h),
                   st["blur"])
    if keys:
        layout, ncell, nslot = _slot_layout(w, h)
        cnt = ctx.debug_fetch(2, frame).view(np.int32)
        slots = ctx.debug_fetch(3, frame).view(np.uint32)
        assert len(cnt) == ncell and len(slots) == nslot, "%s: %d cells, %d slots; restated %d, %d" % (
            tag, len(cnt), len(slots), ncell, nslot)
        for l, (c0, lay) in enumerate(layout):
            for c, (off, cap) in enumerate(lay):
                want = st["cells"][l][c]
                assert len(want) <= cap
                assert cnt[c0 + c] == len(want), "%s: level %d cell %d holds %d keys, restated %d" % (
                    tag, l, c, cnt[c0 + c], len(want))
                R.check_key_set("%s level %d cell %d (buffer 3)" % (tag, l, c),
                                _unpack(slots[off:off + cnt[c0 + c]]), want)
        ocnt = ctx.debug_fetch(5, frame).view(np.int32)
        okeys = ctx.debug_fetch(4, frame).view(np.uint32)
        off, ninis = 0, _n_ini(w, h)
        for l, N in enumerate(st["cfg"]["n_per_level"]):
            assert len(st["selected"][l]) <= max(N + 2, 4 * ninis[l])  # DistributeOctTree's bound
            assert ocnt[l] == len(st["selected"][l]), "%s: level %d keeps %d keys, restated %d" % (
                tag, l, ocnt[l], len(st["selected"][l]))
            R.check_key_set("%s level %d octree (buffer 4)" % (tag, l),
                            _unpack(okeys[off:off + ocnt[l]]), st["selected"][l])
            off += max(N, 4 * ninis[l]) + 8
        assert off == len(okeys) == ctx.capacity()
    assert ctx.debug_fetch(6).view(np.int32)[0] == 0, tag + ": device error flags"


# ------------------------------------------------------------------ the shape table
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_stages_at_tiling_edges(name):
    w, h, why = SHAPES[name]
    assert _accepted(w, h) and why(w, h), "%s (%d x %d) no longer is what it is in the table for" % (
        name, w, h)
    ctx = _ctx(w, h)
    g = _frame(w, h, 21)
    st = _ref(w, h, 21, NF)
    assert sum(len(c) for c in st["cands"]) > 100 and len(st["kps"]) > 50
    k, d = ctx.orb_extract(g)
    _check_buffers(ctx, st, w, h, name)
    R.check_records(name, k, d, st["kps"], st["desc"])
    ctx.close()


def test_one_pixel_below_the_smallest_is_rejected():
    w, h, why = SHAPES["smallest"]
    assert why(w, h)
    for bad in ((w - 1, h), (w, h - 1)):
        assert not _accepted(*bad)
        with pytest.raises(M.MmtError):
            _ctx(*bad)


def test_shape_table_covers_both_paths_of_every_switch():
    """CPU-only bookkeeping: both k_fast instantiations, nIni = 1 and >= 2, a one-row resize band
    and blur band, 1-3 column blur tiles on two levels, both sides of the 1024-column block."""
    tiles = {n: _fast_tile(w, h) for n, (w, h, _) in SHAPES.items()}
    assert min(tiles.values()) <= 40 and max(tiles.values()) == 60
    ninis = set(v for (w, h, _) in SHAPES.values() for v in _n_ini(w, h))
    assert {1, 2} <= ninis
    assert {w % 256 for (w, h, _) in SHAPES.values()} >= {1, 2, 3}
    assert {_lw(w, h)[1] for (w, h, _) in SHAPES.values()} >= {1024, 1025}


# ------------------------------------------------------------------ batches above 32: k_resize
def _pyr_max_frames():
    src = open(os.path.join(os.path.dirname(M.__file__), "csrc", "mmt_internal.h")).read()
    return int(re.search(r"pyr_max_frames_\s*=\s*(\d+)", src).group(1))


@pytest.mark.parametrize("name", ["400x260", "resize_1025", "smallest"])
def test_batch_of_33_takes_the_resize_chain(name, oracle_mod):
    """OrbEngine::run_part builds the pyramid with one k_pyramid launch up to pyr_max_frames_
    frames per call and with the seven-launch k_resize chain above: 33 frames take the chain, the
    first 32 of them k_pyramid, and both must give what the restatement and the oracle give."""
    w, h, why = SHAPES[name]
    assert why(w, h)
    nb = 33
    assert nb - 1 <= _pyr_max_frames() < nb
    frames = [_frame(w, h, 100 + i) for i in range(nb)]
    assert len({f.tobytes() for f in frames}) == nb
    ctx = _ctx(w, h, batch=nb)
    outs = ctx.orb_extract_batch(frames)
    for i in (0, 16, 32):
        R.check_images("%s frame %d of 33, pyramid (k_resize chain)" % (name, i),
                       _split_levels(ctx.debug_fetch(0, i), w, h), R.pyramid(frames[i]))
    assert ctx.debug_fetch(6).view(np.int32)[0] == 0
    for i, (k, d) in enumerate(outs):
        kr, dr = oracle_mod.orb_extract(frames[i], NF)
        R.check_records("%s frame %d of 33" % (name, i), k, d, kr, dr)
    outs32 = ctx.orb_extract_batch(frames[:32])
    for i in (0, 16, 31):
        R.check_images("%s frame %d of 32, pyramid (k_pyramid)" % (name, i),
                       _split_levels(ctx.debug_fetch(0, i), w, h), R.pyramid(frames[i]))
    for i, ((k, d), (k2, d2)) in enumerate(zip(outs, outs32)):
        assert k.tobytes() == k2.tobytes() and d.tobytes() == d2.tobytes(), \
            "%s frame %d: the 33-frame and the 32-frame call differ" % (name, i)
    ctx.close()


# ------------------------------------------------------------------ row stride and device pitch
def _padded(g, stride, fill=0xFF):
    h, w = g.shape
    buf = np.full((h, stride), fill, np.uint8)
    buf[:, :w] = g
    return buf


@pytest.mark.parametrize("name", ["400x260", "blur_w1_l0"])
def test_row_stride_and_device_pitch(name):
    import torch
    w, h, why = SHAPES[name]
    assert why(w, h)
    L = M.lib()
    ctx = _ctx(w, h, batch=2)
    cap = ctx.capacity()
    g0, g1 = _frame(w, h, 31), _frame(w, h, 32)
    packed = ctx.orb_extract_batch([g0, g1])
    R.check_records(name + " packed", packed[0][0], packed[0][1], *R.orb_extract(g0, NF))
    stride = w + 13
    p0, p1 = _padded(g0, stride), _padded(g1, stride)
    # mmt_orb_extract, stride = w + 13, padding 0xFF
    kps = np.zeros(cap, M.KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = ctypes.c_int(0)
    ctx._check(L.mmt_orb_extract(ctx.handle, M._p(p0), w, h, stride, M._p(kps), M._p(desc), cap,
                                 ctypes.byref(n)))
    assert kps[:n.value].tobytes() == packed[0][0].tobytes(), name + ": mmt_orb_extract, stride"
    assert desc[:n.value].tobytes() == packed[0][1].tobytes()
    # mmt_orb_extract_batch
    kps = np.zeros((2, cap), M.KP_DTYPE)
    desc = np.zeros((2, cap, 32), np.uint8)
    ns = np.zeros(2, np.int32)
    ptrs = (ctypes.c_void_p * 2)(p0.ctypes.data, p1.ctypes.data)
    ctx._check(L.mmt_orb_extract_batch(ctx.handle, ptrs, 2, stride, M._p(kps), M._p(desc), cap,
                                       M._p(ns)))
    for f in range(2):
        assert kps[f, :ns[f]].tobytes() == packed[f][0].tobytes(), name + ": batch, stride"
        assert desc[f, :ns[f]].tobytes() == packed[f][1].tobytes()
    # a stride below the width is an error, not a read out of bounds
    with pytest.raises(M.MmtError):
        ctx._check(L.mmt_orb_extract_batch(ctx.handle, ptrs, 2, w - 1, M._p(kps), M._p(desc),
                                           cap, M._p(ns)))
    # mmt_orb_extract_device: frames w * h + 777 bytes apart, the slack 0xFF
    dev = torch.device("cuda:0")
    pitch = w * h + 777
    host = np.full(2 * pitch, 0xFF, np.uint8)
    host[:w * h] = g0.ravel()
    host[pitch:pitch + w * h] = g1.ravel()
    d_gray = torch.from_numpy(host).to(dev)
    d_kps = torch.zeros(2 * cap * M.KP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_desc = torch.zeros(2 * cap * 32, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx._check(L.mmt_orb_extract_device(ctx.handle, d_gray.data_ptr(), 2, pitch, d_kps.data_ptr(),
                                        d_desc.data_ptr(), cap, d_n.data_ptr(), None))
    ctx.orb_device_status()  # synchronises the context stream
    ns = d_n.cpu().numpy()
    kps = d_kps.cpu().numpy().view(M.KP_DTYPE).reshape(2, cap)
    desc = d_desc.cpu().numpy().reshape(2, cap, 32)
    for f in range(2):
        assert kps[f, :ns[f]].tobytes() == packed[f][0].tobytes(), name + ": device, pitch"
        assert desc[f, :ns[f]].tobytes() == packed[f][1].tobytes()
    ctx.close()


# ------------------------------------------------------------------ octree key capacity
NOISE_W, NOISE_H = 504, 378  # smallest 4:3 size (width a multiple of 4) over the capacity


def _noise(w, h):
    return np.random.default_rng(16384).integers(0, 256, (h, w), dtype=np.uint8)


def test_level0_keys_beyond_lds_capacity(oracle_mod):
    """More than 16384 level-0 candidates -- the hard upper bound of key_cap_ in OrbEngine::setup
    -- so k_octree<1> keeps the keys in global scratch, not in LDS."""
    w, h = NOISE_W, NOISE_H
    g = _noise(w, h)
    st = R.orb_stages(g, 1000)
    assert len(st["cands"][0]) > 16384
    assert len(R.level_candidates(_noise(w - 4, h - 3))) <= 16384  # and no smaller size does
    ctx = _ctx(w, h, 1000)
    k, d = ctx.orb_extract(g)
    _check_buffers(ctx, st, w, h, "noise")
    kr, dr = oracle_mod.orb_extract(g, 1000)
    R.check_records("noise against the oracle", k, d, kr, dr)
    R.check_records("noise against the restatement", k, d, st["kps"], st["desc"])
    ctx.close()
