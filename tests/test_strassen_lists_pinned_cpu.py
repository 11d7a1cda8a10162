"""Every list the Strassen planner (sympgpr_amd/csrc/strassen_plan.hip, host code) emits over the grid of tools/strassen_lists.py,
pinned to the digests tests/golden/strassen_lists.json holds: they were written by the build before the planner, the scratch and the
executors got files of their own (python tools/strassen_lists.py --write ...), so a planner that emits one other word anywhere --
a record, a resolved threshold, a schedule annotation, a reserved size -- fails here.  Three child processes (SGPR_GEMM_STRASSEN
unset, = 1, and two sum streams) run side by side; no GPU needed.  `python tools/strassen_lists.py --shapes MODE` finds the call
behind a group that differs."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import strassen_lists as sl  # noqa: E402


@pytest.fixture(scope="module")
def lists():
    with open(os.path.join(ROOT, "tests", "golden", "strassen_lists.json")) as f:
        golden = json.load(f)
    return golden, sl.run_all()


def test_every_list_is_the_pinned_one(lists):
    golden, got = lists
    assert sorted(got) == sorted(golden) == sorted(sl.MODES)
    for mode in sl.MODES:
        assert sorted(got[mode]["digests"]) == sorted(golden[mode]["digests"]), mode
    assert sl.differences(golden, got) == []
    for mode in sl.MODES:
        assert got[mode]["stats"] == golden[mode]["stats"], mode


def test_the_grid_reaches_what_it_is_there_for(lists):
    """a grid that went quiet (tunables that no longer apply, a fetcher that returns nothing) must not pass"""
    _, got = lists
    for mode in ("unset", "streams2"):
        st = got[mode]["stats"]
        print(mode, st)
        assert st["kinds"] == list(range(1, 11))                    # every record kind
        assert st["lists_with_kinds_6_to_9"] >= 1
        assert st["schedules_with_second_buffers"] >= 1
        assert st["capped_lists_that_differ"] >= 1
    # SGPR_GEMM_STRASSEN=1: the library's thresholds, so the top level is off and its lists are pass-through records
    st = got["one"]["stats"]
    print("one", st)
    assert set(st["kinds"]) >= {1, 2, 3, 10} and st["capped_lists_that_differ"] >= 1
    assert got["streams2"]["digests"] != got["unset"]["digests"]    # two sum streams change the schedules
