"""The pass schedule of a loaded plan on the CPU, under AddressSanitizer + UBSan: which ops fold into one launch, every tensor's lifetime under those
launches, and where the activation arena puts it (waifu2x-tensorrt_amd/csrc/schedule.cpp - what load() asks for before it allocates anything).  A mistake
there fails nothing on the device; it lets two live tensors share bytes.

`make asan` builds w2x_parse_check; its `schedule` mode lowers a graph the way load() does (super-batch included), runs candidate_launches() and
layout_arena() and prints one line per plan, op, launch and tensor.  It judges nothing: everything below is recomputed here from the op lines (the tensors
each op reads and writes) and compared with what the library printed.  The graphs are the ones the fold tests of tests/test_gpu_parity.py load."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "waifu2x-tensorrt_amd")
CHECK = os.path.join(PKG, "w2x_parse_check")
ENV = dict(os.environ, ASAN_OPTIONS="exitcode=97:detect_leaks=1:allocator_may_return_null=0:max_allocation_size_mb=2048", UBSAN_OPTIONS="print_stacktrace=1")
UNIT = 3072

GRAPHS = {"swin4": ("swin_unet/art", 4, 2, 64), "cunet2": ("cunet/art", 2, 2, 64), "cunet1": ("cunet/art", 1, 2, 64), "swin4_t256": ("swin_unet/art", 4, 4, 256)}
PRECISIONS = ("fp16", "tf32", "fp32")
VARIANTS = {"default": (), "no_fuse_head": ("no_fuse_head=1",), "no_fuse": ("no_fuse=1",), "check_general": ("check_general=1",)}
# (the tile-256 graph - 48 tiles per pass instead of the small-tile super-batch's 64 - takes 3 s to lower under the sanitizers: its default lists only)
CASES = [(g, p, v) for g in GRAPHS for p in PRECISIONS for v in VARIANTS if v == "default" or g != "swin4_t256"]
SPAN = {"op": 1, "head": 2, "stem": 2, "up": 2, "mlp32": 2, "attn32": 3}


@pytest.fixture(scope="module", autouse=True)
def _built():
    r = subprocess.run(["make", "-C", PKG, "asan"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(CHECK), r.stderr[-2000:]


def check(*args, timeout=120):
    r = subprocess.run([CHECK, *map(str, args)], capture_output=True, timeout=timeout, env=ENV)
    return r.returncode, (r.stdout + r.stderr).decode("utf-8", "replace")


def fields(rest, last):
    """'a=1 b=2 name=x y' -> {'a': '1', 'b': '2', 'name': 'x y'}: the field `last` takes the rest of the line"""
    head, tail = rest.split(f"{last}=", 1)
    d = dict(kv.split("=", 1) for kv in head.split())
    d[last] = tail
    return d


def ids(s):
    return [] if s == "-" else [int(v) for v in s.split(",")]


def parse(out):
    s = {"ops": [], "launches": [], "tensors": []}
    for line in out.splitlines():
        word, _, rest = line.partition(" ")
        if word == "plan":
            s["plan"] = {k: int(v) for k, v in (kv.split("=") for kv in rest.split())}
        elif word == "op":
            i, _, rest = rest.partition(" ")
            d = fields(rest, "name")
            assert int(i) == len(s["ops"])
            s["ops"].append({"kind": d["kind"], "rd": ids(d["rd"]), "wr": ids(d["wr"]), "name": d["name"]})
        elif word == "launch":
            d = fields(rest, "label")
            s["launches"].append({"kind": d["kind"], **{k: int(d[k]) for k in ("first", "last", "timed", "family")}})
        elif word == "tensor":
            t, _, rest = rest.partition(" ")
            assert int(t) == len(s["tensors"])
            s["tensors"].append({k: int(v) for k, v in (kv.split("=") for kv in rest.split())})
        elif word == "arena":
            s["arena"] = {k: int(v) for k, v in (kv.split("=") for kv in rest.split())}
    assert len(s["ops"]) == s["plan"]["ops"] and len(s["tensors"]) == s["plan"]["tensors"] and "arena" in s, out[-2000:]
    return s


@pytest.fixture(scope="module")
def schedule(onnx_model):
    """every case through the driver once, side by side; the tests share the parsed results"""
    paths = {g: onnx_model(model, scale, batch, tile, noise=1) for g, (model, scale, batch, tile) in GRAPHS.items()}

    def one(case):
        graph, prec, variant = case
        rc, out = check("schedule", paths[graph], GRAPHS[graph][2], GRAPHS[graph][3], prec, *VARIANTS[variant])
        assert rc == 0, (case, out[-3000:])
        return case, parse(out)
    with ThreadPoolExecutor(6) as ex:
        done = dict(ex.map(one, CASES))
    return lambda graph, prec, variant: done[(graph, prec, variant)]


def lifetimes(s, launches):
    """everything a launch touches is live over [first, last] of the launch; the input from -1, the output to nops"""
    nops, nt = len(s["ops"]), len(s["tensors"])
    first, last = [nops] * nt, [-1] * nt
    for L in launches:
        for i in range(L["first"], L["last"] + 1):
            for t in s["ops"][i]["rd"] + s["ops"][i]["wr"]:
                first[t] = min(first[t], L["first"])
                last[t] = max(last[t], L["last"])
    first[s["plan"]["in"]] = -1
    last[s["plan"]["out"]] = nops
    return first, last


def roundup(v, unit):
    return (v + unit - 1) // unit * unit


def overlapping_pairs(s, first, last):
    """placed tensors whose closed lifetimes intersect, found by a sweep over the sorted starts"""
    placed = sorted((t for t, d in enumerate(s["tensors"]) if d["placed"]), key=lambda t: first[t])
    for k, a in enumerate(placed):
        for b in placed[k + 1:]:
            if first[b] > last[a]:
                break
            yield a, b


def kinds(s):
    return [L["kind"] for L in s["launches"]]


@pytest.mark.parametrize("graph,prec,variant", CASES)
def test_launches_partition_the_ops(schedule, graph, prec, variant):
    s = schedule(graph, prec, variant)
    nops, out_t = len(s["ops"]), s["plan"]["out"]
    at = 0
    for L in s["launches"]:
        assert L["first"] == at and L["last"] - L["first"] + 1 == SPAN[L["kind"]], L
        assert L["timed"] == (L["first"] + 1 if L["kind"] in ("stem", "up") else L["first"]), L
        for i in range(L["first"], L["last"]):
            assert out_t not in s["ops"][i]["wr"], (L, i)          # (out_override replaces the last op's output only)
        at = L["last"] + 1
    assert at == nops


@pytest.mark.parametrize("graph,prec,variant", CASES)
def test_lifetimes_equal_an_independent_computation(schedule, graph, prec, variant):
    s = schedule(graph, prec, variant)
    first, last = lifetimes(s, s["launches"])
    for t, d in enumerate(s["tensors"]):
        assert (d["first"], d["last"]) == (first[t], last[t]), (t, d, first[t], last[t])


@pytest.mark.parametrize("graph,prec,variant", CASES)
def test_placement_alignment_and_disjointness(schedule, graph, prec, variant):
    s = schedule(graph, prec, variant)
    arena = s["arena"]["bytes"]
    touched = {t for op in s["ops"] for t in op["rd"] + op["wr"]}
    for t, d in enumerate(s["tensors"]):
        assert bool(d["placed"]) == (t in touched), (t, d)
        if d["placed"]:
            assert d["off"] % UNIT == 0 and d["off"] + roundup(d["bytes"], UNIT) <= arena, (t, d, arena)
    # under the candidates' lifetimes, and under those of the ops run one by one (load() may split any candidate back into its ops)
    for launches in (s["launches"], [{"first": i, "last": i} for i in range(len(s["ops"]))]):
        first, last = lifetimes(s, launches)
        for a, b in overlapping_pairs(s, first, last):
            A, B = s["tensors"][a], s["tensors"][b]
            assert A["off"] + roundup(A["bytes"], UNIT) <= B["off"] or B["off"] + roundup(B["bytes"], UNIT) <= A["off"], (a, A, b, B)


@pytest.mark.parametrize("graph,prec,variant", CASES)
def test_group_parts_are_aligned_disjoint_and_fit(schedule, graph, prec, variant):
    """a pass cut into NG tile groups runs each group in its own part of the arena, the layout scaled to 1/NG (engine.cpp group_ptr)"""
    s = schedule(graph, prec, variant)
    arena, B = s["arena"]["bytes"], s["plan"]["B"]
    first, last = lifetimes(s, s["launches"])
    pairs = list(overlapping_pairs(s, first, last))
    ran = 0
    for ng in (2, 3, 4):
        part = (arena // ng + 255) // 256 * 256
        assert s["arena"][f"part{ng}"] == part
        if B % ng:
            continue
        ran += 1
        for t, d in enumerate(s["tensors"]):
            if d["placed"]:
                assert d["off"] % ng == 0 and d["bytes"] % ng == 0 and (d["off"] // ng) % 256 == 0, (ng, t, d)
                assert d["off"] // ng + d["bytes"] // ng <= part, (ng, t, d, part)
        for a, b in pairs:
            A, Bt = s["tensors"][a], s["tensors"][b]
            assert A["off"] // ng + A["bytes"] // ng <= Bt["off"] // ng or Bt["off"] // ng + Bt["bytes"] // ng <= A["off"] // ng, (ng, a, A, b, Bt)
    assert ran, B


@pytest.mark.parametrize("graph,prec,variant", CASES)
def test_launch_kinds_follow_precision_and_switches(schedule, graph, prec, variant):
    s = schedule(graph, prec, variant)
    k = kinds(s)
    if prec == "fp16":
        assert "mlp32" not in k and "attn32" not in k
        if variant == "check_general":
            assert set(k) == {"op"}
    else:
        assert not {"head", "stem", "up"} & set(k)
        fused32 = variant in ("default", "no_fuse_head", "check_general") and prec == "tf32" and graph.startswith("swin")
        if prec == "fp32" or not fused32:
            assert set(k) == {"op"}
        else:
            assert k.count("mlp32") >= 1 and k.count("attn32") >= 1
    if variant == "no_fuse_head":
        want = []
        for L in schedule(graph, prec, "default")["launches"]:
            want += [dict(L, kind="op", first=i, last=i, timed=i) for i in (L["first"], L["last"])] if L["kind"] == "head" else [L]
        got = s["launches"]
        assert [{x: L[x] for x in ("kind", "first", "last", "timed")} for L in got] == [{x: L[x] for x in ("kind", "first", "last", "timed")} for L in want]


@pytest.mark.parametrize("graph", list(GRAPHS))
def test_fold_counts_of_the_fp16_lists(schedule, graph):
    """what tests/test_gpu_parity.py asserts of the loaded engine for these graphs and shapes (its three ..._folded_... tests): swin_unet one stem and the image
    head, cunet two stems and two transposed convolutions at both scales"""
    k = kinds(schedule(graph, "fp16", "default"))
    got = {f: k.count(f) for f in ("stem", "up", "head")}
    want = {"stem": 1, "up": 0, "head": 1} if graph.startswith("swin") else {"stem": 2, "up": 2, "head": 0}
    assert got == want, [L for L in schedule(graph, "fp16", "default")["launches"] if L["kind"] != "op"]


def test_super_batch_of_the_plans(schedule):
    """the driver lowers with lower_for_shape(): B is the engine's - 64 tiles per pass at tile 64, 12 batches of 4 at tile 256"""
    assert (schedule("swin4", "fp16", "default")["plan"]["B"], schedule("swin4", "fp16", "default")["plan"]["userB"]) == (64, 2)
    assert (schedule("swin4_t256", "fp16", "default")["plan"]["B"], schedule("swin4_t256", "fp16", "default")["plan"]["userB"]) == (48, 4)


def test_refusals(onnx_model):
    path = onnx_model("cunet/art", 2, 2, 64, noise=1)
    for args in ((path, 2, 64, "fp16", "no_such_switch=1"), (path, 2, 64, "bf16")):
        rc, out = check("schedule", *args)
        assert rc == 2 and "rejected: " in out and len(out.strip().splitlines()[-1]) > len("rejected: "), (args, out[-2000:])
