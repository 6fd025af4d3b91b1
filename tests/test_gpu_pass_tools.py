"""The per-pass timing tools (tools/<pass>_bench.py) on a tiny frame, in process: every field of every row they print, other than the
timings, equals golden/pass_tools_small.json -- recorded on the MI355X with the same arguments from the tools as they were before
tools/pass_frames.py built their frames, never from the tools under test.  The fixture holds null where a timing stood: there the tool must
report a finite time above 0.  Its "meshlets" is the smallest multiple of 1000 at which the recorded 160 x 96 frames are not empty ones
(visbuffer_decode decodes at least a quarter of the frame, every vsm_resolve frame has a backed page)."""
import importlib
import json
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

with open(os.path.join(ROOT, "tests", "golden", "pass_tools_small.json")) as _f:
    GOLDEN = json.load(_f)

TIMING_KEYS = ("ms_median", "ms_min", "streaming_floor_ms")


def same_but_timings(got, want, where):
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), f"{where}: keys {list(got)} != {list(want)}"
        for k in want:
            if k in TIMING_KEYS:
                assert want[k] is None
                assert isinstance(got[k], float) and math.isfinite(got[k]) and got[k] > 0, f"{where}.{k} = {got[k]}"
            else:
                same_but_timings(got[k], want[k], f"{where}.{k}")
    else:
        assert type(got) is type(want) and got == want, f"{where}: {got!r} != {want!r}"


def test_the_fixture_is_not_of_empty_frames():
    decode, = GOLDEN["rows"]["visbuffer_decode"]
    assert decode["decoded"] * 4 >= decode["pixels"]
    resolve, = GOLDEN["rows"]["vsm_resolve"]
    assert all(frame["backed_pages"] >= 1 for frame in resolve["frames"].values())
    assert GOLDEN["meshlets"] % 1000 == 0 and not GOLDEN["fields_that_differ_between_runs"]


@pytest.mark.parametrize("tool", sorted(GOLDEN["rows"]))
def test_rows_equal_the_recorded_ones(tool):
    size = ["--sizes" if tool == "vsm_pages" else "--size", GOLDEN["size"]]
    argv = size + ["--steps", "2", "--warmup", "1", "--meshlets", str(GOLDEN["meshlets"])] + GOLDEN["extra_arguments"].get(tool, [])
    lines = importlib.import_module(tool + "_bench").main(argv)
    rows = [json.loads(line) for line in lines]
    want = GOLDEN["rows"][tool]
    assert len(rows) == len(want)
    for i, (g, w) in enumerate(zip(rows, want)):
        same_but_timings(g, w, f"{tool}[{i}]")
