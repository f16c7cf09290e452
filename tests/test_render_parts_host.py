"""The pipelined parts of a render() call on the CPU, under AddressSanitizer + UBSan: how render_parts() (waifu2x-tensorrt_amd/csrc/tiles.cpp) cuts a frame's
tiles into parts, the step schedule under it (batch_count, pass_slots, last_pass_live) and the canvas cells of a tile range (tile_range_cells, which
shard_plan() shares).  A different cut returns the same bytes at another speed and with another progress schedule, so no GPU test sees it move.

`make asan` builds w2x_parse_check; its `parts` mode prints the grid, the shards and, per schedule (steps, batch, pass size, parts wanted), the parts.  It
judges nothing.  Here every case is compared with tests/golden/render_parts.json - what the engine's inline code computed before render_parts() took it
over - and checked on its own terms, recomputed from the printed lines.

The cases: the frame sizes tests/test_gpu_pipeline_bytes.py renders (tile 64, x4, blend 1/16; five of them also at 0, 1/32 and 1/8), 1920x1080 at tile 256
at the four blends, and one frame whose blend band reaches the tile stride; each with and without TTA, batch 1-4 and 1-4 parts wanted; the pass size takes
its four values (the batch, four batches, 48, 64) in turn, and all four at 1920x1080 with blend 1/16."""
import json
import os
import subprocess
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "waifu2x-tensorrt_amd")
CHECK = os.path.join(PKG, "w2x_parse_check")
ENV = dict(os.environ, ASAN_OPTIONS="exitcode=97:detect_leaks=1:allocator_may_return_null=0:max_allocation_size_mb=2048", UBSAN_OPTIONS="print_stacktrace=1")
MAX_PARTS = 4


@pytest.fixture(scope="module", autouse=True)
def _built():
    r = subprocess.run(["make", "-C", PKG, "asan"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(CHECK), r.stderr[-2000:]


def rects(s):
    return [] if s == "-" else [[int(v) for v in r.split(",")] for r in s.split(";")]


def ints(rest):
    return {k: int(v) for k, v in (kv.split("=") for kv in rest.split())}


def parse(out):
    g = {"tiles": [], "shards": [], "cases": []}
    for line in out.splitlines():
        word, _, rest = line.partition(" ")
        if word == "grid":
            g.update(ints(rest))
        elif word == "tile":
            i, _, rest = rest.partition(" ")
            assert int(i) == len(g["tiles"])
            g["tiles"].append(ints(rest))
        elif word == "shard":
            head, plan, cells = rest.replace(" cells=", " plan=").split(" plan=")
            g["shards"].append(dict(ints(head), plan=rects(plan), cells=rects(cells)))
        elif word == "case":
            g["cases"].append(dict(ints(rest), part=[]))
        elif word == "part":
            k, _, rest = rest.partition(" ")
            head, cells = rest.split(" rects=")
            assert int(k) == len(g["cases"][-1]["part"])
            g["cases"][-1]["part"].append(dict(ints(head), rects=rects(cells)))
    return g


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "render_parts.json")) as f:
        doc = json.load(f)
    return [dict(zip(doc["fields"], row)) for row in doc["cases"]]


@pytest.fixture(scope="module")
def runs(golden):
    """every grid of the fixture through the driver once, side by side: [(grid key, parsed output, the fixture's cases of that grid in printed order)]"""
    by_grid = defaultdict(list)
    for c in golden:
        by_grid[(c["W"], c["H"], c["T"], c["scale"], c["Tout"], c["overlap"])].append(c)

    def one(item):
        key, cases = item
        W, H, T, S, TO, ov = key
        quads = [v for c in cases for v in (c["steps"], c["userB"], c["B"], c["want"])]
        r = subprocess.run([CHECK, "parts", *map(str, (W, H, T, S, TO, repr(ov), repr(ov), *quads))], capture_output=True, timeout=120, env=ENV)
        assert r.returncode == 0, (key, (r.stdout + r.stderr).decode("utf-8", "replace")[-3000:])
        g = parse(r.stdout.decode())
        assert len(g["cases"]) == len(cases) and len(g["tiles"]) == g["count"] == g["nx"] * g["ny"], key
        return key, g, cases
    with ThreadPoolExecutor(6) as ex:
        return list(ex.map(one, by_grid.items()))


def ceil_div(a, b):
    return -(-a // b)


def pass_slots(tiles, steps, userB, B):
    return ceil_div(ceil_div(tiles * steps, userB), B // userB) * B


def test_fixture_spans_the_axes(golden):
    assert len(golden) >= 300
    assert {c["steps"] for c in golden} == {1, 8} and {c["userB"] for c in golden} == {1, 2, 3, 4} and {c["want"] for c in golden} == {1, 2, 3, 4}
    assert {48, 64} <= {c["B"] for c in golden} and any(c["B"] == c["userB"] for c in golden) and any(c["B"] == 4 * c["userB"] for c in golden)
    assert {0.0, 1 / 32, 1 / 16, 1 / 8} <= {c["overlap"] for c in golden}
    assert min(c["tiles"] for c in golden) <= 8 and max(c["tiles"] for c in golden) >= 120
    assert {len(c["first"]) for c in golden} == {1, 2, 3, 4}


def test_parts_equal_the_inline_cut(runs):
    n = 0
    for key, g, cases in runs:
        for c, got in zip(cases, g["cases"]):
            tag = (key, c["steps"], c["userB"], c["B"], c["want"])
            assert (got["steps"], got["userB"], got["B"], got["want"]) == tag[1:], tag
            assert g["count"] == c["tiles"], tag
            p = got["part"]
            assert got["parts"] == len(p) == len(c["first"]), tag
            assert [q["first"] for q in p] == c["first"], tag
            assert [q["tiles"] for q in p] == [b - a for a, b in zip(c["first"], c["first"][1:] + [c["tiles"]])], tag
            assert [q["batches"] for q in p] == c["batches"] and [q["before"] for q in p] == c["batches_before"], tag
            assert [q["slots_off"] for q in p] == c["slots_off"], tag
            assert (got["batches"], got["slots"], got["x_split"], got["slab"]) == (c["batch_total"], c["slot_total"], c["x_split"], c["slab_slots"]), tag
            if c["rects"] is not None:
                assert [q["rects"] for q in p] == c["rects"], tag
            n += 1
    assert n >= 300


def test_config_3_runs_as_16_20_9(runs):
    """1920x1080, tile 256, x4, blend 1/16, batch 4, three parts: the cut INTEGRATION.md quotes"""
    hits = [got for key, g, cases in runs if key == (1920, 1080, 256, 4, 960, 1 / 16)
            for c, got in zip(cases, g["cases"]) if (c["steps"], c["userB"], c["want"]) == (1, 4, 3)]
    assert len(hits) == 4                                        # (every pass size)
    for got in hits:
        assert [q["tiles"] for q in got["part"]] == [16, 20, 9]


def test_the_cut_on_its_own_terms(runs):
    for key, g, cases in runs:
        W, H, T, S, TO, ov = key
        count, sx, sy = g["count"], TO - g["ovx"], TO - g["ovy"]
        for got in g["cases"]:
            steps, userB, B, want, p = got["steps"], got["userB"], got["B"], got["want"], got["part"]
            tag = (key, steps, userB, B, want)
            # a partition of [0, count) in ascending order
            at = 0
            for q in p:
                assert q["first"] == at and q["tiles"] > 0, tag
                at += q["tiles"]
            assert at == count, tag
            # boundaries at whole reference batches
            unit = next(q for q in range(1, userB + 1) if q * steps % userB == 0)
            assert all(q["first"] % unit == 0 for q in p), tag
            # the schedule: batches, slots
            assert got["batches"] == ceil_div(count * steps, userB) == sum(q["batches"] for q in p), tag
            off = before = 0
            for q in p:
                assert (q["slots_off"], q["before"]) == (off, before), tag
                assert q["batches"] == ceil_div(q["tiles"] * steps, userB) and q["slots"] == pass_slots(q["tiles"], steps, userB, B), tag
                assert q["live"] == q["tiles"] * steps - (q["tiles"] * steps - 1) // B * B and 0 < q["live"] <= B, tag
                off += q["slots"]; before += q["batches"]
            assert got["slots"] == off, tag
            assert got["slab"] == max(p[-1]["first"] * steps + p[-1]["slots"], pass_slots(count, steps, userB, B)), tag
            assert got["slab"] >= count * steps, tag
            # how many parts
            if count < 16 or want <= 1 or g["ovx"] >= sx or g["ovy"] >= sy:
                assert len(p) == 1, tag
            assert len(p) <= max(1, min(want, MAX_PARTS, count // 8)), tag
            body = (count - max(8, count // 5)) // unit * unit
            if len(p) > 1 and p[-1]["first"] == body:
                assert p[-1]["tiles"] >= 8, tag
            # the cells: at most three rectangles per part, pairwise disjoint, covering the canvas
            assert all(1 <= len(q["rects"]) <= 3 for q in p), tag
            cells = [r for q in p for r in q["rects"]]
            assert all(w > 0 and h > 0 and x >= 0 and y >= 0 and x + w <= W * S and y + h <= H * S for x, y, w, h in cells), tag
            for i, (ax, ay, aw, ah) in enumerate(cells):
                for bx, by, bw, bh in cells[i + 1:]:
                    assert ax + aw <= bx or bx + bw <= ax or ay + ah <= by or by + bh <= ay, (tag, cells)
            assert sum(w * h for _, _, w, h in cells) == W * S * H * S, (tag, cells)
            # the split of the upload
            assert 0 < got["x_split"] <= W, tag
            if got["x_split"] < W:
                assert len(p) > 1 and got["x_split"] < W - 64, tag
                assert all(g["tiles"][t]["x"] + T <= got["x_split"] for t in range(p[0]["tiles"])), tag


def test_cells_of_a_tile_range_are_the_shard_plans(runs):
    for key, g, _ in runs:
        W, H, T, S, TO, ov = key
        assert len(g["shards"]) == sum(range(1, 9))
        fits = g["ovx"] < TO - g["ovx"] and g["ovy"] < TO - g["ovy"]
        for parts in range(1, 9):
            sh = [s for s in g["shards"] if s["parts"] == parts]
            assert [s["part"] for s in sh] == list(range(parts))
            assert all(s["owned"] == int(fits) for s in sh), key
            for s in sh:
                if not fits:
                    assert s["tiles"] == 0 and not s["plan"] and not s["cells"], (key, s)
                    continue
                t0, t1 = s["part"] * g["count"] // parts, (s["part"] + 1) * g["count"] // parts
                assert (s["first"], s["tiles"]) == ((t0, t1 - t0) if t1 > t0 else (0, 0)), (key, s)          # (more parts than tiles: a part without a share)
                assert s["halo"] == s["first"] - max(0, s["first"] - g["ny"] - 1), (key, s)
                assert s["plan"] == s["cells"] and (len(s["plan"]) > 0) == (s["tiles"] > 0), (key, s)
            if fits:
                assert sum(w * h for s in sh for _, _, w, h in s["plan"]) == W * S * H * S, key
