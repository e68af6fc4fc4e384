"""Host check of the lifting primitives of the batch bc_feat route (glia_amd/csrc/tree_paths.hpp): cli/tree_paths_check compares the
join-node climb, the path length of every directed entry and the path min / max tables after the push-down with parent-pointer walks,
on a caterpillar of depth 200 (from both ends), a complete binary tree of 256 leaves, a forest with never-merged leaves and random
trees of at most 64 leaves.  No GPU."""
import os
import re
import subprocess

CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cli", "tree_paths_check")


def test_tree_paths_agree_with_parent_pointer_walks():
    if not os.path.exists(CHECK):
        subprocess.check_call(["make", "-C", os.path.dirname(CHECK), "tree_paths_check"], stdout=subprocess.DEVNULL)
    for trees, seed in ((2000, "0x9E3779B97F4A7C15"), (500, "20261019")):
        r = subprocess.run([CHECK, str(trees), seed], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.match(r"tree_paths_check: (\d+) trees, (\d+) nodes, (\d+) entries agree with parent-pointer walks \((\d+) never joined, (\d+) paths hold a root\)", r.stdout)
        assert m, r.stdout
        n_trees, nodes, entries, never, root = (int(g) for g in m.groups())
        # the four fixed trees carry every ordered leaf pair: 2 * 201 * 200 + 256 * 255 + 40 * 39 entries before the random ones
        assert n_trees == trees + 4 and entries > 2 * 201 * 200 + 256 * 255 + 40 * 39 and never > 0 and root > 0
