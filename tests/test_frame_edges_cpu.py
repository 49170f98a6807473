"""The frame-size tests' CPU side: the premises of the frames of tests/edge_frames.py (every oracle frame traced through the square camera is real
work; every frame sits on the side of its guard that its name says; the partition arithmetic of the part pair), the restated decision at the
guards, tools/queue_check on the tile grids of those frames, and the bound of the ticket arithmetic -- tiles x frames < 2^26 -- settled in 64 bits
before any such batch is launched on a GPU."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import edge_frames as E
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _oracle(scene):
    return O.OracleScene(scene)


@functools.lru_cache(maxsize=None)
def _queue_check():
    exe = os.path.join(ROOT, "build", "queue_check")
    subprocess.run(["make", "-s", "build/queue_check"], cwd=ROOT, check=True)
    return exe


# ---------------------------------------------------------------------------------------------------------------- premises
@pytest.mark.parametrize("scene,h,w", [(s, h, w) for s in E.SCENES for (h, w) in E.oracle_sizes()] +
                         [("irreg", f.h, f.w) for f in E.LARGEST] + [("rgbbox",) + E.BOUND_FRAME])
def test_oracle_frames_are_real_work(scene, h, w):
    """Through the square camera every frame has >= 1.5 rays per pixel and >= 1000 pixels with chains of more than 4 rays (the pixels the list's
    short classes and the COLD / SOLO paths serve): conditions that keep a case from becoming empty, not tolerances.  Measured: rgbbox 3.7-4.1
    rays per pixel with chains up to the bounce limit, irreg 1.67-1.68 with chains of 19 (tall frames) to 44 rays."""
    sc = _oracle(scene)
    n = sc.chain_lengths(h, w, cam=sc.camera_floats(*E.SQUARE))
    print(f"{scene} {h} x {w}: {n.sum() / n.size:.3f} rays per pixel, longest chain {n.max()}, {int((n > 4).sum())} pixels with chains > 4")
    assert n.sum() >= 1.5 * n.size
    assert int((n > 4).sum()) >= 1000


def test_the_derived_camera_would_look_at_the_background():
    """Why the square camera: the camera prepare_scene derives for an 8 x 65 535 frame sees next to nothing (about one ray per pixel)."""
    sc = _oracle("rgbbox")
    n = sc.chain_lengths(8, 65535)
    assert n.sum() < 1.01 * n.size


def test_partition_arithmetic_of_the_part_pair():
    """rows_local of a part of two of the 131 056- and 131 072-row images: exactly 65 528 and 65 536, by the restatement, the library
    (rt_part_rows) and the row lists the multi-GPU layer uses; the inside part's GLOBAL rows pass 2^16."""
    from raytracers_amd import api
    from raytracers_amd.dist import tile_rows
    for h, want in zip(E.PART_PAIR, (65528, 65536)):
        for part in (0, 1):
            rows = tile_rows(h, part, 2)
            assert E.part_rows(h, part, 2) == api.part_rows(h, part, 2) == len(rows) == want
            assert rows.max() == h - 8 * (1 - part) - 1 and rows.max() > 65535
        assert sorted(np.concatenate([tile_rows(h, 0, 2), tile_rows(h, 1, 2)]).tolist()) == list(range(h))
    inside, outside = E.PAIRS["list_part_row"]
    assert (E.rows_local(inside), E.rows_local(outside)) == (65528, 65536)
    assert E.tile_grid(inside) == (1, 8191) and E.tile_grid(outside) == (1, 8192)


def test_every_frame_sits_where_its_name_says():
    g = E.tile_grid
    assert g(E.PAIRS["list_column"][0]) == (8192, 1) and E.PAIRS["list_column"][1].w == 1 << 16
    assert g(E.PAIRS["list_row"][0]) == (1, 8192) and E.PAIRS["list_row"][1].h == 1 << 16
    assert g(E.PAIRS["first_order_tiles_y"][0]) == (2, 4096) and g(E.PAIRS["first_order_tiles_y"][1]) == (2, 4097)
    assert g(E.PAIRS["first_order_tiles_x"][0]) == (32768, 2) and g(E.PAIRS["first_order_tiles_x"][1]) == (32769, 2)
    assert [g(f) for f in E.LARGEST] == [(131072, 1), (1, 131072)]
    for h, w in E.REFUSED:
        assert h > 1 << 20 or w > 1 << 20 or h * w > 1 << 30
    assert all(h <= 1 << 20 and w <= 1 << 20 for h, w in E.REFUSED[2:]), "the area case passes the side limit"
    # the batch bound: 131 072 tiles per frame; 511 frames inside, 512 on it; both pass the older limits (4096 frames, 2^31 elements)
    h, w = E.BOUND_FRAME
    tiles = -(-h // 8) * -(-w // 8)
    assert tiles == 131072 and tiles * E.BOUND_INSIDE < E.MAX_POSITIONS == tiles * E.BOUND_OUTSIDE
    assert E.BOUND_OUTSIDE <= 4096 and E.BOUND_OUTSIDE * h * w < 1 << 31
    # ... and why not 1 x 1 frames: a batch has at most 4096 frames, so frames of fewer than 2^14 tiles never reach 2^26 positions; at one
    # pixel of height that takes 2^17 columns, and the first refused batch of any such shape writes 2^29 pixels
    assert 4096 * 1 < E.MAX_POSITIONS and 4096 * (1 << 14) == E.MAX_POSITIONS


def test_no_single_frame_reaches_the_position_bound():
    """ceil(h / 8) ceil(w / 8) <= h w / 64 + (h + w) / 8 + 1 <= 2^24 + 2^18 + 1 under the size limits: the bound concerns batches only."""
    worst = max(-(-h // 8) * -(-w // 8) for h, w in [(1 << 20, 1 << 10), (1 << 15, 1 << 15), (1, 1 << 20), ((1 << 10) + 1, (1 << 20) - 1023), (32769, 32767)])
    assert worst <= (1 << 24) + (1 << 18) + 1 < E.MAX_POSITIONS


# ---------------------------------------------------------------------------------------------------------------- the restated decision
def test_expected_decisions_at_the_guards():
    """The restatement gives the guarded path on every inside frame and not on its outside twin, for both kinds of scene."""
    for lds in (True, False):
        kinds = lambda f, **o: [E.expected(f, k, lds, **o).tickets for k in (1, 2, 3, 4)]
        for name in ("list_column", "list_row", "list_part_row"):
            inside, outside = E.PAIRS[name]
            # (their first frames are rasters: one tile row, or more than 4096 of them)
            assert kinds(inside) == ["tiles-raster"] + ["pixel-list"] * 3, name
            assert "pixel-list" not in kinds(outside) and kinds(outside)[1:] == ["tiles-ordered"] * 3, name
            assert E.expected(inside, 1, lds).recording == 2 and E.expected(outside, 1, lds).recording == 1
        for name in ("first_order_tiles_y", "first_order_tiles_x"):
            inside, outside = E.PAIRS[name]
            assert kinds(inside)[0] == "tiles-bit-reversed" and kinds(outside)[0] == "tiles-raster", name
        assert kinds(E.PAIRS["first_order_tiles_y"][0])[1] == "pixel-list", "8 192 tiles: within the list's gates"
        assert kinds(E.PAIRS["first_order_tiles_x"][0])[1] == "tiles-ordered", "65 536 tiles: beyond px_max_tiles, and w >= 65 536"
        # strips: no list, no first order
        for f in E.SIXTEEN_BIT:
            assert kinds(f, xcd_queues=1) == ["tiles-raster"] + ["tiles-ordered"] * 3
            assert kinds(f, xcd_queues=0) == kinds(f)
            assert kinds(f, pixel_order=0)[1:] == ["tiles-ordered"] * 3
            assert kinds(f, pixel_order=2) == kinds(f)
            assert kinds(f, first_order=0)[0] == "tiles-raster"
        for f in E.LARGEST:
            assert kinds(f) == ["tiles-raster"] + ["tiles-ordered"] * 3
            assert E.expected(f, 1, lds).wide == (not lds), "the wide shape: only for a scene that is read from L2"
    assert E.wide_launch(256) == (1280, 4) and E.wide_launch(255) == (1272, 4)
    s = ("family=pooled tickets=pixel-list instantiation=ORD+SOLO frames=1 tiles=8192 grid=256 waves=16 counters=8(turns) deep_class=0 deep_split=0 "
         "recording=0 nodes=planes")
    got = E.parse_launch(s)
    assert (got.tickets, got.instantiation, got.tiles, got.grid, got.waves, got.counters, got.turns, got.recording) == ("pixel-list", "ORD+SOLO", 8192, 256, 16, 8, True, 0)
    assert E.parse_launch("family=pixel").family == "pixel" and E.parse_launch("family=pixel").tickets is None


# ---------------------------------------------------------------------------------------------------------------- the ticket queue
def test_tile_queue_at_the_extreme_grids():
    """tools/queue_check extreme: the grids 1 x 8192, 8192 x 1, 1 x 131 072, 131 072 x 1, 32 768 x 2 and 2 x 4096 under one counter, eight strips and
    eight counters taking turns, with 4096 and with 5120 waves, and a batch of each: every slot handed out exactly once, and under strips the
    grids narrower than eight tiles leave 8 - tiles_x shards empty whose counters nobody touches."""
    out = subprocess.run([_queue_check(), "extreme"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "queue_check: 48 extreme cases passed" in out.stdout
    for grid in ("1x8192", "8192x1", "1x131072", "131072x1", "32768x2", "2x4096"):
        lines = [l for l in out.stdout.splitlines() if l.startswith(f"ok: {grid} tiles")]
        assert len(lines) == 8, grid
        assert sum("a strip each" in l for l in lines) == 2 and sum("taking turns" in l for l in lines) == 2 and sum("3 frame(s)" in l for l in lines) == 2
        assert sum("5120 waves" in l for l in lines) == 4


def _span(ntiles, nframes, ds, tpt, n_deep=0, n_split=0):
    out = subprocess.run([_queue_check(), "span"] + [str(v) for v in (ntiles, nframes, ds, tpt, n_deep, n_split)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"span: positions=(\d+) tickets=(\d+) tickets32=(\d+) differ=(\d+)(?: first=(\d+) got=\[(\d+),(\d+)\) want=\[(\d+),(\d+)\))?", out.stdout)
    assert m, out.stdout
    return [None if v is None else int(v) for v in m.groups()]


@pytest.mark.parametrize("tpt", [0, 2])
def test_ticket_spans_overflow_from_2_to_the_26_positions(tpt):
    """ticket_span's q_next / q_end are (position) * 64 in 32-bit unsigned: every ticket of a launch against the same formula in uint64_t.
    Found: they agree for 2^26 - 1 positions; at 2^26 the LAST ticket's q_end is 2^32 and wraps to 0 (one ticket differs); at 2^26 + 1
    position 2^26 itself starts at 2^32 -> 0, the slots of position 0 (two tickets differ).  So a pooled launch is refused unless
    tiles per frame x frames < 2^26 (api.cpp: enqueue_render) -- this test examines the arithmetic, not that guard."""
    below, at, above = (_span((1 << 26) + d, 1, 0, tpt) for d in (-1, 0, 1))
    assert below[3] == 0 and below[1] == below[2]
    last = ((1 << 26) - 1) >> tpt
    assert at[3] == 1 and at[4] == last and at[6] == 0 and at[8] == 1 << 32 and at[5] == at[7], at
    assert above[3] == 2 and above[4] == last, above
    # the same through the shape a refused batch would have had: 131 072 tiles x 512 frames, split and deep tiles at its head
    assert _span(131072, 512, 2, tpt, 100, 10)[3] == 1 and _span(131072, 511, 2, tpt, 100, 10)[3] == 0
