"""Generates tests/golden/reference/runs.npz: what the reference's own code (oracle/_ref/*, `make -C oracle ref`) prints and
writes for every input tests/test_oracle_vs_ref.py and tests/test_cabi_host.py feed it (tests/_refruns.py keys each run by
its program, arguments, environment and input digests).  The tests run once against the live binaries while they are
recorded, so a recording is only written from a passing run.  Data only: stdout and output files as bytes.

usage (from the repo root, after `make -C oracle ref`):  python tests/golden/reference/make_runs.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "runs.npz")
TESTS = ["tests/test_oracle_vs_ref.py", "tests/test_cabi_host.py"]

with tempfile.TemporaryDirectory() as d:
    env = dict(os.environ, GLIA_REF_RECORD=d)
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider"] + TESTS, cwd=ROOT, env=env)
    runs = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            runs[name] = np.frombuffer(f.read(), np.uint8)
np.savez_compressed(OUT, **runs)
print("%s: %d entries, %d bytes" % (os.path.relpath(OUT, ROOT), len(runs), os.path.getsize(OUT)))
