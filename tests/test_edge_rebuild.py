"""Host check of the rule that rebuilds an edge record of the window queue from a list entry (glia_amd/csrc/edge_record.hpp):
cli/edge_rebuild_check lays five regions out as adj_fill_fat does and compares every rebuilt record, byte for byte, with the sixteen
words store_new_edge writes for an edge created at or above the horizon.  No GPU."""
import os
import re
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cli", "edge_rebuild_check")


def test_records_rebuilt_from_list_entries_match_the_stored_form():
    if not os.path.exists(CHECK):
        subprocess.check_call(["make", "-C", os.path.dirname(CHECK), "edge_rebuild_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"edge_rebuild_check: (\d+) records rebuilt from list entries agree with the stored form \(cat 0/1/2: (\d+)/(\d+)/(\d+)\)", r.stdout)
    assert m, r.stdout
    n, c0, c1, c2 = (int(g) for g in m.groups())
    assert n == 8 and c0 + c1 + c2 == n and min(c0, c1, c2) > 0          # every edge of the graph, every category of update_seq
