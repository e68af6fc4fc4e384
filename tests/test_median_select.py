"""Host check of the selection core of the median layout (glia_amd/csrc/median_select.hpp): cli/median_select_check compares the
order statistic selected over signed sorted runs with std::nth_element on the materialised multiset difference.  No GPU."""
import os
import re
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cli", "median_select_check")


def test_selection_over_signed_runs_matches_nth_element():
    if not os.path.exists(CHECK):
        subprocess.check_call(["make", "-C", os.path.dirname(CHECK), "median_select_check"], stdout=subprocess.DEVNULL)
    for cases, seed in ((4000, "0x9E3779B97F4A7C15"), (2000, "20250614")):
        r = subprocess.run([CHECK, str(cases), seed], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.match(r"median_select_check: (\d+) cases agree with nth_element \((\d+) with subtracted runs, (\d+) one-element sets\), (\d+) empty", r.stdout)
        assert m, r.stdout
        agree, diff, single, empty = (int(g) for g in m.groups())
        # every kind of case was met: differences, one-element sets and empty sets (which the callers answer with 0 themselves)
        assert agree + empty == cases and agree > cases // 2 and diff > cases // 4 and single > 0 and empty > 0
