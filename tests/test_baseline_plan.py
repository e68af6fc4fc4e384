"""Host check of what the pb-mean window queue decides on the host at its set-up and at every baseline
(glia_amd/csrc/baseline_plan.hpp): the number of saliency cells, the bits the sort by seq looks at, the lanes per list and the slots of
the collection pass, and the interval and horizon of the next launch.  cli/baseline_plan_check holds the expected values as literals
worked out by hand -- a run of four baselines (first one, a descent of 10 cells, no descent, not more than 4096 items), a top within
delta of cell 0, the same with GLIA_HMT_REBASE_END = 1, with the horizon off and with GLIA_HMT_REBASE unset.  No GPU."""
import os
import re
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cli", "baseline_plan_check")


def test_the_plan_of_a_baseline_matches_values_worked_out_by_hand():
    if not os.path.exists(CHECK):
        subprocess.check_call(["make", "-C", os.path.dirname(CHECK), "baseline_plan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"baseline_plan_check: (\d+) plans, (\d+) cell counts, (\d+) seq-bit counts, (\d+) lane choices and (\d+) slot counts agree", r.stdout)
    assert m, r.stdout
    plans, cells, bits, lanes, slots = (int(g) for g in m.groups())
    # the run of 4 and the top near cell 0, twice; the five with the horizon off; the two default intervals
    assert plans == 5 + 5 + 5 + 2 and cells == 5 and bits == 4 and lanes == 9 and slots == 4
