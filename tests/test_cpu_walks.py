"""The cases of tests/test_gpu_walks.py held to their preconditions without a GPU: every case gives the loop it is meant
for a second trip under the caps of include/magnify_hip.h as they stand, stays within the size limit, and the case list
and DESIGN.md's table ("Capped launches and who walks them twice") name the same loops."""
import os
import re

import pytest

import walk_shapes as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", ws.CASES, ids=lambda c: c.id)
def test_the_case_takes_its_loop_round_again(case):
    count, groups = ws.require_second_trip(case)
    assert groups >= 1 and count > groups
    assert case.loop in ("items", "planes")
    if case.loop == "planes":
        assert groups == ws.MAX_Y  # the only way a plane loop strides: more planes than a grid's y


@pytest.mark.parametrize("case", ws.CASES, ids=lambda c: c.id)
def test_the_case_stays_small(case):
    assert 0 < case.device_bytes <= ws.GIB, case.id


def test_the_walk_caps_come_from_the_header():
    names = [k for k in ws.D if "_WALK" in k]
    assert len(names) >= 30 and all(isinstance(ws.D[k], int) and ws.D[k] > 0 for k in names)
    assert ws.MAX_Y == 65535
    # a raised budget turns a precondition red instead of sending its case back to one trip: the shapes of the cases
    # are fixed numbers, so the table below is what a header with that budget gives
    case = ws.BY_ID["mg_bin_planes-items-uint8-bin2"]
    old = ws.D["MG_BIN_WALK"]
    try:
        ws.D["MG_BIN_WALK"] = 2 * old
        with pytest.raises(AssertionError, match="one trip"):
            ws.require_second_trip(case)
    finally:
        ws.D["MG_BIN_WALK"] = old
    ws.require_second_trip(case)


def test_plane_grid_is_mg_plane_grid():
    assert ws.plane_grid(27, 256, 4096, 64) == (16, 256)
    assert ws.plane_grid(27, 4, 4096, 64) == (27, 4)
    assert ws.plane_grid(500, 4, 4096, 64) == (64, 4)
    assert ws.plane_grid(3, 70000, 4096) == (1, 65535)  # never below one workgroup a plane
    assert ws.plane_grid(10000, 3) == (10000, 3)


def design_rows():
    """(entries, walk, taken by) of every row of DESIGN.md's table."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text.split("Capped launches and who walks them twice", 2)[1].split("\n## ")[0]
    rows = []
    for line in section.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if not line.startswith("|") or len(cells) != 6 or cells[0] in ("Entry", "---"):
            continue
        rows.append((re.findall(r"`(mg_\w+)`", cells[0]), cells[2], cells[5]))
    return rows


def test_design_table_and_case_list_name_the_same_loops():
    """A row given to test_gpu_walks.py states how many cases take it ("(2 cases)"), or names the entry whose case
    takes it along; the counts of an entry's walk add up to its cases in walk_shapes.CASES, and no case is left over."""
    rows = design_rows()
    assert len(rows) >= 40
    stated = {}
    for entries, walk, taken in rows:
        assert walk in ("items", "planes"), (entries, walk)
        # every row names a test, or says why the loop cannot stride
        assert "cannot stride" in taken or re.search(r"test_\w+\.py", taken), entries
        if "test_gpu_walks.py" not in taken:
            continue
        n = re.search(r"test_gpu_walks\.py` \((\d+) cases?\b", taken)
        if n:
            assert entries, taken
            stated[(entries[0], walk)] = stated.get((entries[0], walk), 0) + int(n.group(1))
        else:  # taken along by another entry's case
            assert any(ws.cases_of(e) for e in re.findall(r"`(mg_\w+)`", taken)), (entries, taken)
    have = {}
    for c in ws.CASES:
        have[(c.entry, c.loop)] = have.get((c.entry, c.loop), 0) + 1
    assert stated == have, sorted(set(stated.items()) ^ set(have.items()))
