"""Host check of the merge-order validator bc_feat and bc_label share (glia_amd/csrc/dense_order.hpp): cli/dense_order_check compares it
with a model that keeps the set of live keys merge by merge -- the dense pairs of random valid orders over 1 to 64 sparse ascending
labels, and for each order corrupted in five ways (unknown region, already merged, reused created key, created key equal to a leaf,
n == R) the kind of the failure and the index of the first offending merge.  Its second line: leaf_truth_counts of the same header, the
labels of a contingency table -> leaves, against a map lookup per entry, with every kind of entry it drops.  No GPU."""
import os
import re
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cli", "dense_order_check")


def test_dense_order_agrees_with_the_live_key_model():
    if not os.path.exists(CHECK):
        subprocess.check_call(["make", "-C", os.path.dirname(CHECK), "dense_order_check"], stdout=subprocess.DEVNULL)
    for orders, seed in ((2000, "0x9E3779B97F4A7C15"), (500, "20261019")):
        r = subprocess.run([CHECK, str(orders), seed], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.match(r"dense_order_check: (\d+) orders, (\d+) merges agree with the live-key model; corrupted: (\d+) unknown, (\d+) merged, (\d+) reused, "
                     r"(\d+) leaf key, (\d+) too many", r.stdout)
        assert m, r.stdout
        n_orders, merges, unknown, merged, reused, leaf, too_many = (int(g) for g in m.groups())
        # every order gets the n == R corruption; the others need one merge (unknown, leaf key) or two (merged, reused) to corrupt
        assert n_orders == orders and too_many == orders and merges > 10 * orders
        assert unknown == leaf and merged == reused and orders // 2 < merged <= unknown <= orders
        # second line: leaf_truth_counts (the table of label_overlap -> the (leaf, truth) table of bc_label) against a map lookup per entry
        m = re.match(r"leaf_truth_counts: (\d+) tables, (\d+) entries agree with the map lookup; kept: (\d+) \((\d+) with truth 0, (\d+) with truth 0xFFFFFFFF\); "
                     r"dropped: (\d+) below, (\d+) between, (\d+) above the labels, (\d+) masked, (\d+) reserved pair$", r.stdout.splitlines()[1])
        assert m, r.stdout
        tables, entries, kept, truth0, truth_max, below, between, above, masked, reserved = (int(g) for g in m.groups())
        assert tables == orders and entries == kept + below + between + above + masked + reserved
        assert min(truth0, truth_max, below, between, above, masked, reserved) > 0 and kept > 10 * orders
