"""One table per kernel family states what is built, and its predicate and its launcher read it (csrc/dq_launch.h).
The forms every shape takes are pinned against tests/golden/launch_forms.json (tools/launch_forms.py: the device-free query entries,
recorded under the library from before the tables); the greps keep the shared host pieces in their one place.  No GPU."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffusion-deconvolution-dia-msms-data_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_forms.json")
# the files whose launchers go through DQ_INST tables
TABLE_FILES = ("k_level.hip", "k_tiny.hip", "k_conv_wg.hip", "k_res_cp.hip", "k_res_rows.hip", "k_res_wg.hip", "k_res.hip", "k_la_small.hip",
               "k_la_rows_fwd.hip", "k_la_rows_bwd.hip", "k_la_long.hip", "k_linattn.hip", "k_la_bwd.hip", "k_conv.hip")


def _files_with(pattern):
    names = sorted(n for n in os.listdir(CSRC) if n.endswith((".hip", ".cpp", ".h")))
    return [n for n in names if re.search(pattern, open(os.path.join(CSRC, n)).read())]


def test_forms_match_the_golden_sweep():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import launch_forms
    finally:
        sys.path.pop(0)
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    assert sum(len(v) for v in golden.values()) > 20000  # (the whole sweep, not a stub)
    assert launch_forms.differences(golden, launch_forms.sweep()) == []


def test_cu_count_is_queried_in_one_place():
    assert _files_with(r"multiProcessorCount|MultiprocessorCount") == ["dq_api.hip"]


def test_occupancy_is_queried_in_one_place():
    assert _files_with(r"hipOccupancyMaxActiveBlocksPerMultiprocessor") == ["dq_api.hip"]


def test_no_launch_macro_left_in_the_table_files():
    for name in TABLE_FILES:
        text = open(os.path.join(CSRC, name)).read()
        assert re.findall(r"#\s*define\s+DQ_\w+", text) == [], name
        assert "DQ_INST(" in text and "find_inst(" in text, name
