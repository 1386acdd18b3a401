"""Prints the float32 twin's floors of tests/pose_rows_ref.py (FLOOR of tests/test_gpu_pose_edges.py) and of durf_pose_finish.
Run from the repository root: python tests/scripts/pose_rows_floors.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import pose_rows_ref as PR      # noqa: E402

if __name__ == '__main__':
    for kind, cases in (('obj', PR.OBJ_CASES), ('bkgd', PR.BKGD_CASES)):
        for case in cases:
            print("    ('%s', %r, %r, %r): (%s)," % ((kind,) + case + (', '.join('%.1e' % f for f in PR.twin_floor(kind, case)),)))
    for name, f in sorted(PR.finish_floors().items()):
        print("    %r: %.1e," % (name, f))
