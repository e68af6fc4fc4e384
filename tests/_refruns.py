"""Runs of the reference's own code (oracle/_ref/*, built in place by `make -C oracle ref` where the reference's sources are
available), recorded for the exact inputs the tests feed them: tests/golden/reference/runs.npz.

A run is keyed by the program, its arguments, the environment it is given and digests of its stdin and input files, so a
recorded answer is only ever used for the input it was recorded from.  Order of lookup: with GLIA_REF_RECORD=<dir> the
binary runs and its output is also written to <dir> (tests/golden/reference/make_runs.py packs them); otherwise the
recording; otherwise the binary, if it is built.  An input with neither is a test failure, never a skip.
"""
import hashlib
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference", "runs.npz")
_recorded = None


def _sha(b):
    return hashlib.sha1(b).hexdigest()


def _key(exe, args, stdin, files, outputs, env):
    desc = repr((exe, tuple(args), sorted(env.items()), _sha(stdin), sorted((n, _sha(b)) for n, b in files.items()), tuple(outputs)))
    return _sha(desc.encode())


def _live(exe, args, stdin, files, outputs, env):
    with tempfile.TemporaryDirectory() as d_in, tempfile.TemporaryDirectory() as d_out:
        for name, data in files.items():
            with open(os.path.join(d_in, name), "wb") as f:
                f.write(data)
        argv = [os.path.join(BIN, exe)] + [a.replace("{in}", d_in).replace("{out}", d_out) for a in args]
        res = subprocess.run(argv, input=stdin, capture_output=True, check=True, env=dict(os.environ, **env))
        out = {}
        for name in outputs:
            with open(os.path.join(d_out, name), "rb") as f:
                out[name] = f.read()
    return res.stdout, out


def run(exe, args=(), stdin="", files=None, outputs=(), env=None):
    """exe: a program under oracle/_ref.  `{in}` / `{out}` in args name a directory holding `files` ({name: bytes}) / one the
    program writes `outputs` (names) into.  -> (stdout as text, {output name: bytes})"""
    global _recorded
    args, files, env = [str(a) for a in args], dict(files or {}), dict(env or {})
    stdin = stdin.encode() if isinstance(stdin, str) else bytes(stdin)
    key = _key(exe, args, stdin, files, outputs, env)
    record = os.environ.get("GLIA_REF_RECORD")
    if record:
        stdout, out = _live(exe, args, stdin, files, outputs, env)
        os.makedirs(record, exist_ok=True)
        for name, data in [("", stdout)] + sorted(out.items()):
            with open(os.path.join(record, key + ("." + name if name else "")), "wb") as f:
                f.write(data)
        return stdout.decode(), out
    if _recorded is None:
        _recorded = {}
        if os.path.exists(FIXTURE):
            with np.load(FIXTURE) as z:
                _recorded = {k: z[k] for k in z.files}
    if key in _recorded:
        return _recorded[key].tobytes().decode(), {name: _recorded[key + "." + name].tobytes() for name in outputs}
    if os.path.exists(os.path.join(BIN, exe)):
        stdout, out = _live(exe, args, stdin, files, outputs, env)
        return stdout.decode(), out
    raise AssertionError("no recorded run of oracle/_ref/%s for this input (and the binary is not built): "
                         "tests/golden/reference/make_runs.py records them" % exe)
