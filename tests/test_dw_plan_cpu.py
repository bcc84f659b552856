"""CPU: the K-split plan of the fused weight-gradient entry, read from the library (sn_weight_grads_plan: host only, the plan
sn_weight_grads hands to its kernels) -- its coverage property at every accepted size up to 8192 rows and a few large ones, and that
the row counts of tests/test_weight_grads_edges_gpu.py reach the K-range edges they are there for."""
import ctypes

import pytest

from sinnerf_amd import _lib
from tests.helpers import DW_EDGE_ROWS, DW_EDGE_WRAP_ROWS, dw_edge_reach, dw_plan

CODES = {"fp32": _lib.SN_DTYPE_F32, "bf16": _lib.SN_DTYPE_BF16, "bf16_state": _lib.SN_DTYPE_BF16_STATE,
         "bf16_state_emb16": _lib.SN_DTYPE_BF16_STATE | _lib.SN_DTYPE_EMB_BF16, "bf16x3": _lib.SN_DTYPE_BF16X3}
SIZES = list(range(16, 8192 + 1, 16)) + [16384 + 16, 65536, 524288, 4096 * 192 + 16]
# variant -> (m, n): the `Task` comment of csrc/sn_dw_common.h (6 / 7 = 1 / 3 with the embedded inputs stored as bf16)
SHAPES = {0: (256, 256), 1: (256, 64), 2: (128, 256), 3: (128, 64), 4: (32, 256), 5: (32, 128), 6: (256, 64), 7: (128, 64)}
FLAGS = {"fp32": 0, "bf16": 0x100, "bf16_state": 0x300, "bf16_state_emb16": 0x300, "bf16x3": 0x500}
MAX_GRID = 2 ** 31 - 1                                    # workgroups of a one-dimensional launch


@pytest.mark.parametrize("mode", list(CODES))
def test_every_point_lies_in_exactly_one_non_empty_range(mode):
    code = CODES[mode]
    for rows in SIZES:
        plan = dw_plan(rows, code)
        assert isinstance(plan, list) and len(plan) == 14, (rows, plan)
        nbytes = _lib.lib.sn_weight_grads_workspace_bytes(rows, code)
        assert nbytes > 0
        intervals, tasks = [], {}
        for i, q in enumerate(plan):
            at = (mode, rows, i, q)
            assert q["variant"] & ~0xff == FLAGS[mode] and (q["m"], q["n"]) == SHAPES[q["variant"] & 0xff], at
            assert (q["variant"] & 0xff in (6, 7)) == (mode == "bf16_state_emb16" and i in (0, 5, 11)), at
            assert q["ns"] >= 1, at
            assert q["per"] % (32 if code & 0xff == _lib.SN_DTYPE_BF16_STATE and q["variant"] & 0xff == 0 else 16) == 0, at
            # every point in exactly one range, and no range empty (an empty task would leave its partial unwritten)
            assert (q["ns"] - 1) * q["per"] < rows <= q["ns"] * q["per"], at
            assert q["group"] in (0, 1) and q["first"] >= 0, at
            tasks.setdefault(q["group"], []).append((q["first"], q["first"] + q["ns"]))
            intervals.append((q["c_off"], q["c_off"] + q["ns"] * q["m"] * q["n"] * 4))
            assert (q["b_off"] is not None) == (i not in (5, 11, 12)), at              # skip / direction columns and sigma share a bias
            if q["b_off"] is not None:
                intervals.append((q["b_off"], q["b_off"] + q["ns"] * q["m"] * 4))
        # the 256 x 256 problems of the modes with a kernel of their own run as launch group 0, everything else as group 1
        two = mode in ("fp32", "bf16_state", "bf16_state_emb16")
        assert sorted(tasks) == ([0, 1] if two else [0]), (mode, rows)
        for q in plan:
            assert q["group"] == (1 if two and q["variant"] & 0xff != 0 else 0), (mode, rows, q)
        for g, spans in tasks.items():                                                  # contiguous from 0, no overlap
            spans.sort()
            assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (mode, rows, g, spans)
            assert 0 < spans[-1][1] <= MAX_GRID, (mode, rows, g)
        intervals.sort()
        assert intervals[0][0] >= 0 and all(a[1] <= b[0] for a, b in zip(intervals, intervals[1:])), (mode, rows, intervals)
        assert intervals[-1][1] <= nbytes, (mode, rows)


def test_plan_entry_checks_its_arguments_like_the_workspace_query():
    L = _lib.lib
    buf = (ctypes.c_int32 * (9 * 14))()
    for mode, code in CODES.items():
        for rows in (0, 8, 100, -16):
            assert L.sn_weight_grads_plan(rows, code, buf, 14) == -5 == L.sn_weight_grads_workspace_bytes(rows, code), (mode, rows)
    for code in (7, _lib.SN_DTYPE_F16, 0x40):                                           # unknown / inference-only dtype codes
        assert L.sn_weight_grads_plan(4096, code, buf, 14) == -4 == L.sn_weight_grads_workspace_bytes(4096, code), code
    for code in (_lib.SN_DTYPE_F32, _lib.SN_DTYPE_BF16, _lib.SN_DTYPE_BF16X3):          # emb16 belongs to the bf16 state alone
        code |= _lib.SN_DTYPE_EMB_BF16
        assert L.sn_weight_grads_plan(4096, code, buf, 14) == -4 == L.sn_weight_grads_workspace_bytes(4096, code), code
    assert L.sn_weight_grads_plan(8, 7, buf, 14) == -5                                  # the shape is looked at first, as there
    assert L.sn_weight_grads_plan(4096, 0, None, 14) == -1 and L.sn_weight_grads_plan(4096, 0, buf, -1) == -1
    # a short buffer receives the first problems only
    for i in range(len(buf)):
        buf[i] = -77
    assert L.sn_weight_grads_plan(4096, 0, buf, 3) == 14
    assert all(v != -77 for v in buf[:27]) and all(v == -77 for v in buf[27:])
    assert L.sn_weight_grads_plan(4096, 0, None, 0) == 14


@pytest.mark.parametrize("mode", list(CODES))
def test_edge_sweep_reaches_every_short_range(mode):
    """The row counts of the GPU edge tests, as a whole, put every chunk count 1..8 into a FIRST and into a LAST K-range, in each
    launch group and for the 256 x 256 problems, and wrap the narrow problems' 16-deep ring at the large size (the same assertion
    runs in front of the GPU tests: a retuned cost table that moves the ranges fails here first)."""
    reach, longest_narrow = dw_edge_reach(CODES[mode])
    assert ("variant0",) in reach and ("group", 0) in reach
    for key, (first, last) in reach.items():
        assert first >= set(range(1, 9)), (mode, key, "first", sorted(first))
        assert last >= set(range(1, 9)), (mode, key, "last", sorted(last))
    assert longest_narrow > 16, (mode, longest_narrow)
    assert DW_EDGE_WRAP_ROWS in DW_EDGE_ROWS
