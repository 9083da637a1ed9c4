"""The activation selection's entry points are declared, exported and bound (no GPU), in the manner of
tests/test_abi.py."""
import re
import subprocess

from ldso_amd import _lib as L
from test_abi import CT_HEADER, HEADER, declared_symbols

CT_SYMBOLS = ("ldso_ct_make_distance_map", "ldso_ct_make_distance_map_ba", "ldso_ct_select_activation",
              "ldso_ct_immature_append", "ldso_ct_selection_download")
BA_SYMBOLS = ("ldso_ba_activate_points_tracker",)


def test_activation_selection_symbols(built):
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (ldso_\w+)", out))
    ct_declared, ba_declared = declared_symbols(CT_HEADER, "ldso_ct_"), declared_symbols(HEADER, "ldso_ba_")
    ct_bound, ba_bound = {n for n, _, _ in L.CT_ABI}, {n for n, _, _ in L.ABI}
    for s in CT_SYMBOLS:
        assert s in ct_declared and s in exported and s in ct_bound, s
    for s in BA_SYMBOLS:
        assert s in ba_declared and s in exported and s in ba_bound, s
    lib = L.lib()
    assert lib.ldso_ct_select_activation(None, None, None, 0, None, None, None, None) < 0
    assert b"null context" in lib.ldso_ba_last_error()
    assert lib.ldso_ba_activate_points_tracker(None, 0, None, 1, None) < 0
    assert lib.ldso_ct_num_kernels() == 7  # the new launches take no timing slot


def test_python_face():
    from ldso_amd import BAContext
    from ldso_amd.tracker import CoarseTracker

    for name in ("make_distance_map", "make_distance_map_ba", "select_activation", "immature_append"):
        assert callable(getattr(CoarseTracker, name))
    assert callable(BAContext.activate_points_tracker)
    assert (L.ACT_KEEP, L.ACT_DELETE, L.ACT_OPTIMIZE) == (0, 1, 2)
