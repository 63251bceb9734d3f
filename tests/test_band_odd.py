"""The N > 1 band frame away from the benchmark shapes, on the CPU: the cases of helpers.BAND_ODD_CASES reach what they
are meant to reach, HaloFrame's plan partitions every one of them, and the Python rehearsal over gloo gives the
one-process frame.

The cases are the ones the native frame (rsd_band_frame_front / _back, csrc/band_frame.cpp) is to run on the GPU:
helpers.ODD_FRAMES and one tall frame, worlds 2, 3, 5 and one more than the frame has 32-row groups, both SD splits,
the default sample reach (ssMaxRadius 512 px: every window is the whole map) and a reach of 24 px.  A green
bit-equality test means nothing if no texel travels or the plan never leaves its even path, so this module checks the
inputs on the oracle and on HaloFrame._plan alone (BandFrame::plan is written to be the same plan).  No test runs the
native frame on these cases (it hangs where a rank has nothing to exchange);
tests/test_gpu_band_odd.py holds the communicator's tests.

  * per case with at least two ranks that own rows, some rank's pass 1 touches at least 30 SD texels that another rank
    traces -- the exchange carries data;
  * over the table: a rank without a 32-row group, a `tiles` region whose last tile is partial, a `tiles` region that
    starts on another tile than its window's first, a window that neither map edge clips, an AO band whose byte offset
    or length is no multiple of 16, and a last band that carries guard-band rows of pass 1's padded dispatch.

These are conditions on the inputs, not measurements: a case that misses one is replaced, the condition stays.

Per case the plan's pixel bands and SD shares partition the frame and the map exactly once, every texel a rank's pass 1
touches lies in its window, and every touched texel outside its own share lies in exactly one send region.  The plan's
arithmetic is restated: the rows under a band start on the 8-row tile at or above the band's first SD row, the window is
floor(a / div) + sdGuard - 1 to floor(b / div) + sdGuard + 2 clipped to the map, and a tiled region starts on the first
tile of its peer at or after the window's first tile.  (The reach bound leaves 6 rows or more between the last touched
texel and an unclipped window end on these frames, so the touched texels alone do not pin the window's ends.)

The rehearsal (HaloFrame over the oracle, one process per rank, gloo, at the reach of 24 px): worlds 2 and 3 on
odd_div3, one_over and tiny with both splits, three frames, every rank's AO of the whole frame buffer and its SD share
bit for bit the one-process oracle frame.  Only the world-2 runs of odd_div3 and one_over start from a skewed split
([0, 2, 3] instead of [0, 1, 3]): at world 3 their three groups allow the even split alone, and tiny has one group.

The moving scenes a band frame is to be run over: neighbouring steps of the dynamic sequence and of the animated one differ on at least
100 SD texels and 100 AO pixels, so a frame that carried stale state across an update could not pass there."""
import dataclasses
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from helpers import (BAND_MOVING_WORLD, BAND_ODD_CASES, BAND_REACH_SMALL, BAND_REACH_WHOLE, BAND_TALL_FRAME, ODD_FRAMES,
                     BandOddCase, OracleBackend, band_case_id, band_dynamic_steps, band_frame_shape, band_moving_config,
                     band_odd_backend, band_odd_worlds, band_plans, band_region_rows, band_touched, free_port,
                     odd_frame_config, turnstile_steps)

_IDS = [band_case_id(c) for c in BAND_ODD_CASES]
_backends, _cases = {}, {}


def _backend(O, c):
    """One oracle backend (G-buffer included) per (frame, reach)."""
    if (c.frame, c.reach) not in _backends:
        _backends[c.frame, c.reach] = band_odd_backend(O, c)
    return _backends[c.frame, c.reach]


def _case(O, c):
    """The plans of every rank and the texels each rank's pass 1 touches, computed once per case."""
    if c not in _cases:
        be = _backend(O, c)
        plans = band_plans(be, c.world, c.sd_split)
        touched = [band_touched(be, p.px_rows[r]) for r, p in enumerate(plans)]
        _cases[c] = (be, plans, touched)
    return _cases[c]


def _owner_map(plans, sd_h):
    """Per SD row the rank that traces it, -1 where none does and -2 where more than one does."""
    owner = np.full(sd_h, -1)
    for r, p in enumerate(plans):
        for lo, hi in p.owned_sd_rows():
            owner[lo:hi] = np.where(owner[lo:hi] == -1, r, -2)
    return owner


def test_case_table():
    """Every odd frame at worlds 2, 3, 5 and one more than its groups; both splits; each reach with each split."""
    for f in ODD_FRAMES:
        assert {c.world for c in BAND_ODD_CASES if c.frame == f.name} == set(band_odd_worlds(f)), f.name
        assert max(band_odd_worlds(f)) > -(-f.visible_h // 32)
    assert {(c.sd_split, c.reach) for c in BAND_ODD_CASES} == {(s, r) for s in ("tiles", "rows")
                                                               for r in (BAND_REACH_WHOLE, BAND_REACH_SMALL)}
    assert len(set(BAND_ODD_CASES)) == len(BAND_ODD_CASES) <= 24
    assert BAND_TALL_FRAME.visible_h % 32 and BAND_TALL_FRAME.visible_w % 8


@pytest.mark.parametrize("c", BAND_ODD_CASES, ids=_IDS)
def test_exchange_carries_data(oracle, c):
    """With two or more ranks that own rows, some rank's pass 1 touches at least 30 SD texels another rank traces."""
    be, plans, touched = _case(oracle, c)
    owner = _owner_map(plans, be.sd_h)
    busy = [r for r, p in enumerate(plans) if p.px_rows[r][1] > p.px_rows[r][0]]
    foreign = [int(touched[r][owner != r].sum()) for r in range(c.world)]
    print(f"{band_case_id(c)}: touched {[int(t.sum()) for t in touched]}, of them in another rank's share {foreign}")
    if len(busy) >= 2:
        assert max(foreign) >= 30, foreign
    else:
        assert band_frame_shape(c.frame).visible_h <= 32  # one group: only `tiny`


def test_table_reaches_the_plan_edges(oracle):
    """Over the table, each edge of BandFrame::plan's arithmetic occurs at least once."""
    seen = dict.fromkeys(("empty rank", "partial last tile", "region off the window's first tile", "unclipped window",
                          "AO band off 16 bytes", "last band with guard rows"), 0)
    for c in BAND_ODD_CASES:
        be, plans, _ = _case(oracle, c)
        cfg, p0 = be.cfg, plans[0]
        if any(hi == lo for lo, hi in p0.px_rows):
            seen["empty rank"] += 1
        for r, p in enumerate(plans):
            if c.sd_split == "tiles":
                for k, reg in p.iv_send.items():
                    if not reg:
                        continue
                    rows = band_region_rows(p, reg)
                    last_tile = [y for y in rows if y // 8 == rows[-1] // 8]
                    if len(last_tile) < 8:
                        seen["partial last tile"] += 1
                    if reg[0] // 8 != p.window[r][0] // 8:
                        seen["region off the window's first tile"] += 1
            lo, hi = p.window[r]
            if 0 < lo and hi < be.sd_h and p.px_rows[r][1] > p.px_rows[r][0]:
                seen["unclipped window"] += 1
        row_bytes = be.np_ao[0].nbytes
        if any((lo * row_bytes) % 16 or ((hi - lo) * row_bytes) % 16 for lo, hi in p0.ao_rows if hi > lo):
            seen["AO band off 16 bytes"] += 1
        V, g = cfg.visible_h, cfg.guard_band
        last = max(hi for _, hi in p0.ao_rows)
        if V % 32 and g and last == min(cfg.fb_h, g + 32 * p0.G) and last > g + V:
            seen["last band with guard rows"] += 1
    print(seen)
    assert all(seen.values()), seen


@pytest.mark.parametrize("c", BAND_ODD_CASES, ids=_IDS)
def test_plan_partitions(oracle, c):
    be, plans, touched = _case(oracle, c)
    world, sd_h, p0 = c.world, be.sd_h, plans[0]
    # the pixel bands partition [0, 32 G), the same on every rank
    assert p0.px_rows[0][0] == 0 and p0.px_rows[-1][1] == 32 * p0.G
    assert all(p0.px_rows[r][1] == p0.px_rows[r + 1][0] for r in range(world - 1))
    assert all(lo % 32 == 0 and lo <= hi for lo, hi in p0.px_rows)
    assert all(p.px_rows == p0.px_rows and p.sd_rows == p0.sd_rows and p.window == p0.window for p in plans)
    # the SD shares partition the map's rows exactly once
    assert (_owner_map(plans, sd_h) >= 0).all(), _owner_map(plans, sd_h)
    owner = _owner_map(plans, sd_h)
    # the rows under a band start on an 8-row tile (rsd_sd_trace_rows takes no other boundary) at or above the SD row
    # of the band's first frame-buffer row, less than a tile above it
    cfg = be.cfg
    g, div, sdg = cfg.guard_band, cfg.divisor, int(be.vao.sdGuard)
    for r in range(1, world):
        first = (g + p0.px_rows[r][0]) // div + sdg
        assert p0.sd_rows[r][0] % 8 == 0 or p0.sd_rows[r][0] == sd_h, (r, p0.sd_rows)
        assert p0.sd_rows[r][0] == max(p0.sd_rows[r - 1][0], min(sd_h, first - first % 8)), (r, p0.sd_rows, first)
    for r, p in enumerate(plans):
        lo, hi = p.window[r]
        # the window restated: the SD rows of the frame-buffer rows within halo_px of the band (floor division, also
        # of a negative row), one row more below and, with the end exclusive, two more above, clipped to the map
        a_px = g + p.px_rows[r][0] - p.halo_px
        b_px = g + min(p.px_rows[r][1], cfg.visible_h) + p.halo_px
        assert (lo, hi) == (max(0, int(np.floor(a_px / div)) + sdg - 1), min(sd_h, int(np.floor(b_px / div)) + sdg + 2))
        if c.sd_split == "tiles":
            # a region towards k: from the first tile of k at or after the window's first tile to the window's end
            for k, reg in p.iv_send.items():
                t = next(t for t in range(lo // 8, lo // 8 + world) if t % world == k)
                assert reg == ((8 * t, hi) if 8 * t < hi else None), (r, k, reg, (lo, hi))
        rows = np.flatnonzero(touched[r].any(axis=1))
        # what r's pass 1 touches lies inside its window ...
        assert rows.size == 0 or (lo <= rows.min() and rows.max() < hi), (r, p.window[r], rows.min(), rows.max())
        # ... and outside its own share in exactly one send region
        sends = np.zeros(sd_h, int)
        for k, reg in p.iv_send.items():
            got = band_region_rows(p, reg)
            assert all(owner[y] == k for y in got), (r, k, reg)
            sends[got] += 1
        foreign = rows[owner[rows] != r]
        assert (sends[foreign] == 1).all(), (r, foreign, sends)
        assert (sends <= 1).all() and (sends[owner == r] == 0).all()
        # what r sends to k is what k expects from r
        for k, q in enumerate(plans):
            if k != r:
                assert p.iv_send[k] == q.iv_recv[r] and p.sd_recv[k] == q.sd_send[r]


# ---- the rehearsal over gloo

def _skew(G, world):
    """A first split that is not the even one, where every rank can have a group and another split exists."""
    even = [G * r // world for r in range(world + 1)]
    skew = [0] + [G - (world - 1) + k for k in range(world - 1)] + [G]
    return skew if G >= world and skew != even else None


def _worker(rank, world, port, out_dir, frame, sd_split):
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    for p in (str(root), str(root / "ray-traced-stochastic-depth-map_amd"), str(root / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from oracle import oracle as O
    from rsd.shard import HaloFrame
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    be = band_odd_backend(O, BandOddCase(frame, world, sd_split, BAND_REACH_SMALL))
    f = HaloFrame(be, rank, world, sd_split=sd_split)
    skew = _skew(f.G, world)
    if skew:
        f.gb = skew
        f._plan()
    for i in range(3):
        be.np_ao[:] = 0
        f.frame()
        np.save(os.path.join(out_dir, f"ao_{rank}_{i}.npy"), be.np_ao)
        np.save(os.path.join(out_dir, f"sd_{rank}_{i}.npy"), be.np_sd)
        np.save(os.path.join(out_dir, f"sdrows_{rank}_{i}.npy"), np.array(f.owned_sd_rows()).reshape(-1, 2))
    np.save(os.path.join(out_dir, f"split_{rank}.npy"), np.array(f.splits))
    dist.barrier()
    dist.destroy_process_group()


_refs = {}


def _one_process_frame(O, frame):
    if frame not in _refs:
        from rsd.shard import BandFrame
        ref = band_odd_backend(O, BandOddCase(frame, 1, "rows", BAND_REACH_SMALL))
        BandFrame(ref, 0, 1).frame()
        assert (ref.np_st != 0).any() and (ref.np_rmax != 0).any()
        _refs[frame] = ref
    return _refs[frame]


@pytest.mark.parametrize("sd_split", ["tiles", "rows"])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("frame", ["odd_div3", "one_over", "tiny"])
def test_halo_rehearsal_equals_one_process(oracle, tmp_path, frame, world, sd_split):
    ref = _one_process_frame(oracle, frame)
    mp.start_processes(_worker, args=(world, free_port(), str(tmp_path), frame, sd_split), nprocs=world, join=True,
                       start_method="spawn")
    splits = np.load(tmp_path / "split_0.npy")
    G = -(-band_frame_shape(frame).visible_h // 32)
    if _skew(G, world):
        assert list(splits[0]) == _skew(G, world)
    for r in range(world):
        assert np.array_equal(splits, np.load(tmp_path / f"split_{r}.npy")), "the ranks disagree on the split"
        for i in range(3):
            assert np.array_equal(np.load(tmp_path / f"ao_{r}_{i}.npy"), ref.np_ao), f"rank {r} frame {i}: AO"
            sd = np.load(tmp_path / f"sd_{r}_{i}.npy")
            for lo, hi in np.load(tmp_path / f"sdrows_{r}_{i}.npy"):
                assert np.array_equal(sd[:, lo:hi].view(np.uint32), ref.np_sd[:, lo:hi].view(np.uint32)), \
                    f"rank {r} frame {i}: SD rows {lo}-{hi}"


# ---- the moving scenes of the GPU half

def _oracle_frames(O, scene, steps):
    from rsd.shard import BandFrame
    out = []
    for name, pos in steps:
        be = OracleBackend(O, dataclasses.replace(scene, positions=pos), band_moving_config(), whole_config=True)
        BandFrame(be, 0, 1).frame()
        out.append((name, be.np_sd.copy(), be.np_ao.copy(), int((be.np_rmax != 0).sum())))
    return out


@pytest.mark.parametrize("kind", ["dynamic", "turnstile"])
def test_moving_steps_differ(oracle, kind):
    """Neighbouring steps' oracle frames differ on at least 100 SD texels and 100 AO pixels: a band frame that carried
    the previous step's stamps, ray table or halo buffers across the update would not give the next step's frame."""
    if kind == "dynamic":
        from rsd.scenes import make_scene
        scene = make_scene("arcade_tiny")
        steps = band_dynamic_steps(scene)
    else:
        scene, steps = turnstile_steps()
    frames = _oracle_frames(oracle, scene, steps)
    cfg = band_moving_config()
    assert -(-cfg.visible_h // 32) >= BAND_MOVING_WORLD
    for (a, sd_a, ao_a, live_a), (b, sd_b, ao_b, _) in zip(frames[:-1], frames[1:]):
        sd_diff = int((sd_a.view(np.uint32) != sd_b.view(np.uint32)).any(axis=(0, 3)).sum())
        ao_diff = int((ao_a != ao_b).sum())
        print(f"{kind}: {a} -> {b}: {sd_diff} SD texels, {ao_diff} AO pixels differ ({live_a} touched texels at {a})")
        assert live_a >= 300
        assert sd_diff >= 100 and ao_diff >= 100, (a, b, sd_diff, ao_diff)


def test_odd_configs_are_the_renderers():
    """helpers.odd_frame_config of the tall frame: the SD map size written beside it."""
    from rsd.frame import make_vao
    _, sd_w, sd_h = make_vao(odd_frame_config(BAND_TALL_FRAME))
    assert (sd_w, sd_h) == (26, 109)
