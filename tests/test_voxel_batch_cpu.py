"""The voxel batch without a GPU: the C ABI's new symbols on the three sides, and the conditions the GPU tests rest on --
the members of the batch use different numbers of pair-sum workgroups, and in the float32 restatement of the loop
(tests/voxel_pyramid_reference.py) they end at different iterations and, on the four-level schedule, are at different levels at the same
iteration."""
import os
import re
import subprocess

import numpy as np
import pytest

import voxel_batch_cases as bc
import voxel_pyramid_reference as vpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# symbol -> its arguments as the header declares them, by kind: p = pointer, i = int32_t, l = int64_t
NEW_SYMBOLS = {
    "icpmi_voxel_register_batch_dev": "pipppippp",
    "icpmi_voxel_register_batch": "pipppippp",
    "icpmi_voxel_register_multistart_dev": "pplppiippp",
    "icpmi_voxel_register_multistart": "pplppiippp",
    "icpmi_get_voxel_batch_report": "pipppp",
    "icpmi_debug_voxel_batch_calls": "pp",
}


def _kind_of_c(arg):
    arg = arg.strip()
    if "*" in arg or "[" in arg or arg.startswith("icpmi_handle"):
        return "p"
    if arg.startswith("int32_t"):
        return "i"
    if arg.startswith("int64_t"):
        return "l"
    raise AssertionError(arg)


def _kind_of_ctypes(t):
    import ctypes as C
    if t is C.c_int32:
        return "i"
    if t is C.c_int64:
        return "l"
    assert t is C.c_void_p or issubclass(t, C._Pointer), t
    return "p"


def test_header_library_and_bindings_agree_on_the_new_symbols():
    from norlab_icp_mapper_amd import _capi
    header = open(os.path.join(ROOT, "include", "icpmi.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", _capi.LIB_PATH], text=True).splitlines() if ln.strip()}
    bound = {name: (res, args) for name, res, args in _capi.SYMBOLS}
    import ctypes as C
    for sym, kinds in NEW_SYMBOLS.items():
        m = re.search(r"icpmi_status\s+%s\s*\(([^;]*)\)\s*;" % sym, header)
        assert m, sym
        assert "".join(_kind_of_c(a) for a in m.group(1).split(",")) == kinds, sym
        assert sym in exported, sym
        assert sym in bound, sym
        res, args = bound[sym]
        assert res is C.c_int and "".join(_kind_of_ctypes(t) for t in args) == kinds, sym


def test_members_use_different_numbers_of_workgroups():
    rds = bc.members()
    assert [r.shape[0] for r, _ in rds] == [2000, 600, 257, 1] and all(n.shape == (r.shape[0], 3) for r, n in rds)
    assert [bc.acc_blocks(r.shape[0]) for r, _ in rds] == [8, 3, 2, 1]
    assert bc.acc_blocks(0) == 1 and bc.acc_blocks(256) == 1 and bc.acc_blocks(10 ** 6) == 256
    # prefixes of readings moved by different starts: no two members share their first point
    firsts = {tuple(r[0]) for r, _ in rds[:3]}
    assert len(firsts) == 3
    assert len(bc.SIXTEEN) == 16 and bc.priors().shape == (4, 4, 4) and np.array_equal(bc.priors()[3], np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("sizes", bc.HANDLES)
def test_members_end_at_different_iterations_in_float32(sizes):
    runs = [bc.reference_member(n, k, sizes) for n, k in bc.MEMBERS[:3]]      # (the one-point member has no well-posed float32 reference)
    its = [r["iterations"] for r in runs]
    print(sizes, its, [vpr.report(r) for r in runs])
    assert all(r["status"] == "ok" for r in runs)
    assert len(set(its)) == 3


def test_members_are_at_different_levels_on_the_four_level_schedule():
    reports = [vpr.report(bc.reference_member(n, k, bc.FOUR)) for n, k in bc.MEMBERS[:3]]
    shortest = min(sum(its for its, _, _ in rep) for rep in reports)
    mixed = [i for i in range(1, shortest + 1) if len({bc.levels_at(rep, i) for rep in reports}) > 1]
    print(reports, mixed)
    assert mixed
    assert bc.levels_at([(2, 0, 0), (3, 0, 0)], 2) == 0 and bc.levels_at([(2, 0, 0), (3, 0, 0)], 3) == 1 and bc.levels_at([(2, 0, 0)], 3) is None
