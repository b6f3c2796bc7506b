"""Host tests of the work distribution of the persistent row-owner kernels: the stand-alone enumeration of the index maps
(tools/work_plan_host_check.cpp over csrc/mdx_plan.h, the header the kernels compile) and the library's host exports of the plan.
No GPU."""
import pytest

from moldiff_amd import _lib
from tests import util as U


def test_index_maps_enumerated_by_the_host_check(tmp_path):
    """every unit exactly once and every section bit exactly once for the static plan, the queue's item map, the pairs' ranges, the
    XCD remap and the equal split -- built from the real header with the host compiler"""
    U.run_host_check('work_plan_host_check', tmp_path)


def test_work_plan_export_is_the_launchers_plan():
    # the point the full-size tests land on: 154,666 edges, 9,667 units on 2,048 slots (exact) -- 4 full rounds, split 2 with m = 3
    assert _lib.work_plan(154666 // 16 + 1, 2048) == dict(nslots=2048, nf=4, rem=1475, split=2, m=3)
    assert _lib.work_plan(154666 // 16 + 1, 2048, can_split=False) == dict(nslots=2048, nf=4, rem=1475, split=0, m=0)
    for rem, split, m in ((0, 0, 0), (1, 1, 1), (12, 1, 1), (13, 1, 2), (16, 1, 2), (17, 2, 3), (18, 2, 3), (19, 2, 4), (20, 2, 5), (21, 0, 0),
                          (23, 0, 0)):
        assert _lib.work_plan(48 + rem, 24) == dict(nslots=24, nf=2, rem=rem, split=split, m=m), rem
    with pytest.raises(RuntimeError):
        _lib.work_plan(5, 0)


def test_launch_units_of_a_batch():
    """[24, 31, 18]: 552 + 930 + 306 = 1,788 directed edges; graph-aligned 16-edge units 35 + 59 + 20 = 114 in either order"""
    bn, hei, bh, ei, be = U.graph_from_sizes([24, 31, 18])
    lu = _lib.launch_units(ei, bn, 3, 3)
    assert lu['edge_a_exact'] == dict(nunits=114, grid=6, npairs=3, short=0, equal=0, long1=0, long2=3)      # two workgroups per CU
    assert lu['edge_a_split'] == dict(nunits=57, grid=3, npairs=3, short=0, equal=0, long1=3, long2=0)       # two units per item, one per CU
    assert (lu['edge_b_exact']['nunits'], lu['edge_b_split']['nunits']) == (112, 56)                         # 16 / 32 consecutive edges
    assert lu['bwd_exact']['nunits'] == lu['bwd_split']['nunits'] == 114
    whole = _lib.launch_units(ei, bn, 3, 256)
    assert whole['edge_a_exact']['grid'] == 29 and whole['edge_a_exact']['npairs'] == 29 and whole['edge_a_exact']['short'] == 29
    # a grid between #CUs and 2 #CUs: pairs of two workgroups and pairs of one
    bn, hei, bh, ei, be = U.graph_from_sizes([2, 9, 17, 3, 5, 7])
    a = _lib.launch_units(ei, bn, 6, 5)['edge_a_exact']
    assert a['grid'] > a['npairs'] == 5 and a['long1'] >= 1
    # the launchers read the cap: what they would do "right now" is what they do on a device of that many compute units
    with _lib.cu_cap(3):
        assert _lib.launch_units(ei, bn, 6) == _lib.launch_units(ei, bn, 6, 3)
        with _lib.cu_cap(1):
            assert _lib.launch_units(ei, bn, 6) == _lib.launch_units(ei, bn, 6, 1)
        assert _lib.launch_units(ei, bn, 6) == _lib.launch_units(ei, bn, 6, 3)
    assert _lib.launch_units(ei, bn, 6) != _lib.launch_units(ei, bn, 6, 3)       # restored: the device's own count (256 without one)
    # empty batch: nothing is launched
    bn, hei, bh, ei, be = U.graph_from_sizes([])
    assert all(v['nunits'] == 0 and v['grid'] == 0 for v in _lib.launch_units(ei, bn, 0, 4).values())
