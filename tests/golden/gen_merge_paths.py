"""Generates tests/golden/sshmt/merge_paths.npz: merge orders with the merge paths the REFERENCE'S OWN bounded genMergePaths
(hmt/tree_build.hxx:150-180) writes for them.  A driver written here -- it reads "n max min" and n key triples from standard input and
prints one path per line -- is compiled against that header in place, into a temporary directory outside the repository; nothing
compiled and none of the reference's text is kept.  The header needs no ITK: -std=c++11 and the reference's code directory suffice.

Orders: the oracle's pb-mean order of synth 32^3 at S = 8 (G = 32), random forests (several roots) and caterpillars of up to 600 merges,
a balanced tree; lengths (max, min): (3, 2), (2, 1), (5, 3).  tests/test_sshmt_host.py reads the fixture only.

    python tests/golden/gen_merge_paths.py [reference code directory]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DRIVER = r"""
#include <cstdio>
#include <cstdint>
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>
#include "hmt/tree_build.hxx"
int main() {
  int n, mx, mn;
  if (scanf("%d %d %d", &n, &mx, &mn) != 3) return 1;
  std::vector<glia::TTriple<uint32_t>> order(n);
  for (auto& m : order) if (scanf("%u %u %u", &m.x0, &m.x1, &m.x2) != 3) return 1;
  std::vector<std::vector<int>> paths;
  glia::hmt::genMergePaths(paths, order, mx, mn);
  for (auto const& p : paths) { for (int i : p) printf("%d ", i); printf("\n"); }
  return 0;
}
"""
LENGTHS = [(3, 2), (2, 1), (5, 3)]


def orders():
    import _sshmt_cases as K
    from oracle import pyoracle as O
    labels, pb = O.synth((32, 32, 32), 8, 32)
    out = {"synth32_pb_mean": O.Rag(labels, only_contour=True).merge_order_pb(pb, type=2)[0]}
    for n, R, seed in ((5, 9, 1), (120, 150, 2), (600, 700, 3), (599, 601, 4)):
        out["forest_%d_%d" % (n, R)] = K.forest(n, R, seed)
    for n in (1, 2, 3, 64, 600):
        out["caterpillar_%d" % n] = K.caterpillar(n, key0=n)
    out["balanced_6"] = K.balanced(6)
    return {k: np.ascontiguousarray(v, dtype=np.uint32).reshape(-1, 3) for k, v in out.items()}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("GLIA_REFERENCE_CODE", "")
    assert os.path.isfile(os.path.join(ref, "hmt", "tree_build.hxx")), "give the reference's code directory"
    fixture = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-O1", "-std=c++11", "-I" + ref, src, "-o", exe])
        for name, order in orders().items():
            fixture["order_" + name] = order
            for mx, mn in LENGTHS:
                text = "%d %d %d\n" % (len(order), mx, mn) + "\n".join("%d %d %d" % tuple(m) for m in order.tolist()) + "\n"
                out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
                paths = [[int(v) for v in line.split()] for line in out.splitlines() if line.strip()]
                fixture["offsets_%s_%d_%d" % (name, mx, mn)] = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
                fixture["members_%s_%d_%d" % (name, mx, mn)] = np.array([i for p in paths for i in p], np.int64)
    os.makedirs(os.path.join(HERE, "sshmt"), exist_ok=True)
    np.savez_compressed(os.path.join(HERE, "sshmt", "merge_paths.npz"), **fixture)
    print("wrote %d orders x %d length settings" % (len(fixture) // (1 + 2 * len(LENGTHS)), len(LENGTHS)))


if __name__ == "__main__":
    main()
