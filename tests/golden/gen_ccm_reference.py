"""Generates tests/golden/ccm/ccm_reference.npz: what the REFERENCE'S OWN tree inference of segment_ccm computes for a set of merge
orders and merge probabilities.  A small driver (the text below, ours) is compiled in a temporary directory against the reference's
headers in place -- hmt/tree_build.hxx (genTree) and hmt/tree_ccm.hxx (computeEnergyTuples, resolveFactorTree,
computeFactorNodeEnergyPositive / Negative); the driver restates, in its own words, the node payload and the energy rule of the tool that
calls them (hmt/main_segment_ccm.cxx:12-15,39-53,76-86: the member names are the interface those headers read) -- and its output is recorded: per node the tree arrays, own energies, tuples, pos / neg / confidence, and the picks.
Doubles travel as bit patterns.  tests/test_tree_ccm.py compares the library with the recorded file and never needs the reference.

    python tests/golden/gen_ccm_reference.py [reference code directory, default: $GLIA_REFERENCE or the REF of oracle/Makefile]

Cases (tests/test_tree_ccm.py relies on them): balanced trees, pure chains, random orders of 2 - 400 leaves, partial orders whose tree
is a forest (the root is the last node, as in the reference); probabilities uniform, exactly 0 and 1, within FEPS of either (the isfeq
branches and the FMAX saturation), all 0.5 (every Em == Es tie), all 1, all 0.
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ccm", "ccm_reference.npz")      # a directory of its own: tests/test_golden_cpu.py takes every tests/golden/*.npz for a volume

DRIVER = r"""
// stdin: nCases; per case: nMerges, nMerges lines "x0 x1 x2", nMerges probabilities (%la)
// stdout: per case "C nNodes nPicks", per node "label parent child0 child1" + 7 doubles as hex words (em es Em Es pos neg conf), picks
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <queue>
#include "hmt/tree_build.hxx"
#include "hmt/tree_ccm.hxx"
using namespace glia;
using namespace glia::hmt;
// payload of a node: the member names Em / Es / label are the ones hmt/tree_ccm.hxx and genTree's callers read
struct CcmPayload { double Es; double Em; Label label; };
using Tree = TTree<CcmPayload>;
static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }
int main() {
  int nCases;
  if (scanf("%d", &nCases) != 1) return 2;
  for (int c = 0; c < nCases; ++c) {
    int n;
    if (scanf("%d", &n) != 1) return 2;
    std::vector<TTriple<Label>> order(n);
    for (auto& t : order) if (scanf("%u %u %u", &t.x0, &t.x1, &t.x2) != 3) return 2;
    std::vector<double> mergeProbs(n);
    for (auto& p : mergeProbs) if (scanf("%la", &p) != 1) return 2;
    Tree tree;
    size_t used = 0;
    // the rule of hmt/main_segment_ccm.cxx:47-49: a probability that isfeq calls zero costs FMAX, any other its negative logarithm
    auto energy = [](double q) { if (isfeq(q, 0.0)) return FMAX; return -std::log(q); };
    genTree(tree, order, [&](Tree::Node& node, Label r) {
      const bool leaf = node.isLeaf();
      const double q = leaf ? 0.0 : mergeProbs[used++];
      node.data.label = r;
      node.data.Em = leaf ? 0.0 : energy(q);
      node.data.Es = leaf ? FMAX : energy(1.0 - q);
    });
    std::vector<std::pair<double, double>> Ems;
    computeEnergyTuples(Ems, tree);
    std::vector<int> picks;
    resolveFactorTree(picks, tree, Ems);
    printf("C %d %d\n", (int)tree.size(), (int)picks.size());
    for (auto const& node : tree) {
      double pos = computeFactorNodeEnergyPositive(tree, node.self, Ems), neg = computeFactorNodeEnergyNegative(tree, node.self, Ems);
      double sum = neg;
      double conf = pos / stats::plusEqual(sum, pos);
      printf("%u %d %d %d %llx %llx %llx %llx %llx %llx %llx\n", node.data.label, node.parent, node.children.empty() ? -1 : node.children.front(),
             node.children.empty() ? -1 : node.children.back(), bits(node.data.Em), bits(node.data.Es), bits(Ems[node.self].first),
             bits(Ems[node.self].second), bits(pos), bits(neg), bits(conf));
    }
    for (int p : picks) printf("%d\n", p);
  }
  return 0;
}
"""


def order_random(rng, leaves, merges=None, first_label=1):
    """random binary merges over `leaves` regions; merges < leaves - 1 leaves a forest"""
    live = list(range(first_label, first_label + leaves))
    nxt = first_label + leaves
    out = []
    for _ in range(leaves - 1 if merges is None else merges):
        i, j = rng.choice(len(live), 2, replace=False)
        a, b = live[i], live[j]
        live = [x for x in live if x not in (a, b)] + [nxt]
        out.append((a, b, nxt))
        nxt += 1
    return np.array(out, np.uint32).reshape(-1, 3)


def order_chain(leaves):
    out, cur, nxt = [], 1, leaves + 1
    for k in range(2, leaves + 1):
        out.append((cur, k, nxt))
        cur, nxt = nxt, nxt + 1
    return np.array(out, np.uint32).reshape(-1, 3)


def order_balanced(leaves):
    level, nxt, out = list(range(1, leaves + 1)), leaves + 1, []
    while len(level) > 1:
        up = []
        for i in range(0, len(level) - 1, 2):
            out.append((level[i], level[i + 1], nxt))
            up.append(nxt)
            nxt += 1
        if len(level) % 2:
            up.append(level[-1])
        level = up
    return np.array(out, np.uint32).reshape(-1, 3)


def probs(rng, kind, n):
    if kind == "uniform":
        return rng.random(n)
    if kind == "half":
        return np.full(n, 0.5)
    if kind == "one":
        return np.ones(n)
    if kind == "zero":
        return np.zeros(n)
    assert kind == "edges"          # exact 0 / 1, within FEPS = 2.22e-16 of either, just outside it, and ordinary values
    pool = np.array([0.0, 1.0, 1e-16, 2.2e-16, 2.3e-16, 1e-300, 1.0 - 1.1102230246251565e-16, 1.0 - 2.220446049250313e-16,
                     1.0 - 4.440892098500626e-16, 0.5, 0.25, 0.9])
    p = pool[rng.integers(0, len(pool), n)]
    plain = rng.random(n) < 0.4
    p[plain] = rng.random(int(plain.sum()))
    return p


def cases():
    rng = np.random.default_rng(20161)
    out = []
    for leaves in (2, 3, 4, 5, 6, 7, 8, 9, 16, 64, 256):
        for kind in ("uniform", "edges"):
            out.append(("balanced%d_%s" % (leaves, kind), order_balanced(leaves), kind))
    for leaves in (2, 5, 9, 40, 400):
        for kind in ("uniform", "edges"):
            out.append(("chain%d_%s" % (leaves, kind), order_chain(leaves), kind))
    for leaves in (2, 3, 4, 6, 7, 8, 9, 9, 9, 23, 100, 400):
        for kind in ("uniform", "edges"):
            out.append(("random%d_%s_%d" % (leaves, kind, len(out)), order_random(rng, leaves), kind))
    for leaves, merges in ((9, 5), (12, 7), (60, 40), (400, 250)):
        for kind in ("uniform", "edges"):
            out.append(("partial%d_%d_%s" % (leaves, merges, kind), order_random(rng, leaves, merges), kind))
    for kind in ("half", "one", "zero"):
        out.append(("balanced8_" + kind, order_balanced(8), kind))
        out.append(("chain7_" + kind, order_chain(7), kind))
        out.append(("random9_" + kind, order_random(rng, 9), kind))
        out.append(("random120_" + kind, order_random(rng, 120), kind))
        out.append(("partial30_18_" + kind, order_random(rng, 30, 18), kind))
    return [(name, o, probs(rng, kind, len(o))) for name, o, kind in out]


def reference_dir():
    if len(sys.argv) > 1:
        return sys.argv[1]
    if os.environ.get("GLIA_REFERENCE"):
        return os.environ["GLIA_REFERENCE"]
    mk = open(os.path.join(HERE, "..", "..", "oracle", "Makefile")).read()
    return re.search(r"^REF \?= (\S+)", mk, re.M).group(1)


def main():
    ref = reference_dir()
    cs = cases()
    text = ["%d" % len(cs)]
    for _, o, p in cs:
        text.append("%d" % len(o))
        text += ["%d %d %d" % tuple(r) for r in o.tolist()]
        text += [float(x).hex() for x in p]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "ccm_driver.cc"), os.path.join(d, "ccm_driver")
        with open(src, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + ref, "-o", exe, src])
        res = subprocess.run([exe], input="\n".join(text) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    data, at = {"names": np.array([c[0] for c in cs])}, 0
    for name, o, p in cs:
        tag, nn, npk = res[at].split()
        assert tag == "C"
        rows = [r.split() for r in res[at + 1: at + 1 + int(nn)]]
        picks = [int(x) for x in res[at + 1 + int(nn): at + 1 + int(nn) + int(npk)]]
        at += 1 + int(nn) + int(npk)
        data[name + "/order"], data[name + "/probs"] = o, p
        data[name + "/label"] = np.array([int(r[0]) for r in rows], np.uint32)
        for k, key in enumerate(("parent", "child0", "child1")):
            data[name + "/" + key] = np.array([int(r[1 + k]) for r in rows], np.int32)
        for k, key in enumerate(("em", "es", "Em", "Es", "pos", "neg", "conf")):
            data[name + "/" + key] = np.array([struct.unpack("<d", struct.pack("<Q", int(r[4 + k], 16)))[0] for r in rows], np.float64)
        data[name + "/picks"] = np.array(picks, np.int32)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **data)
    print("%s: %d cases, %d bytes" % (OUT, len(cs), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
