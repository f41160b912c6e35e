"""The reference's command-line tools (oracle/_ref/*, compiled by oracle/ref/Makefile from the reference's own sources where that
tree exists) as the tests call them -- or, where they were not built, their recorded answers from tests/golden/ref_tools.npz.

run(argv) stands for subprocess.run(argv, capture_output=True).  Arguments that are absolute paths name files: a file that exists
before the call is an input and enters the call's key by the hash of its bytes, a file the call creates or changes is an output whose
bytes are recorded (and written back on replay).  The key is the tool's name, the other arguments and the input hashes, so the same
call of the same test has the same key on every machine.

With the tools built every call runs them, and a recorded answer for the same key must agree with them.  RR_RECORD_REF_TOOLS=1 (tools
built) adds the calls of a test run to the recording; without the tools a call that was never recorded fails the test."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_tools.npz")
_records = None


def _load():
    global _records
    if _records is None:
        _records = {}
        if os.path.exists(GOLDEN):
            with np.load(GOLDEN, allow_pickle=False) as z:
                for name in z.files:
                    h, part = name.split(".", 1)
                    _records.setdefault(h, {})[part] = z[name].tobytes()
    return _records


def _save():
    flat = {f"{h}.{part}": np.frombuffer(b, np.uint8) for h, r in sorted(_load().items()) for part, b in sorted(r.items())}
    np.savez_compressed(GOLDEN, **flat)


def _read(p):
    with open(p, "rb") as f:
        return f.read()


def run(argv):
    """-> subprocess.CompletedProcess(argv, returncode, stdout bytes, stderr bytes) of the reference tool argv[0]."""
    argv = [str(a) for a in argv]
    paths = [i for i, a in enumerate(argv[1:], 1) if os.path.isabs(a)]
    before = {i: _read(argv[i]) if os.path.isfile(argv[i]) else None for i in paths}
    key = [os.path.basename(argv[0])] + [("@file:" + hashlib.sha256(before[i]).hexdigest() if before[i] is not None else "@new")
                                         if i in before else a for i, a in enumerate(argv[1:], 1)]
    h = hashlib.sha256(json.dumps(key).encode()).hexdigest()[:40]
    rec = _load().get(h)
    if os.path.exists(argv[0]):
        p = subprocess.run(argv, capture_output=True)
        got = {"meta": json.dumps({"key": key, "rc": p.returncode}).encode(), "stdout": p.stdout}
        for i in paths:
            if os.path.isfile(argv[i]) and _read(argv[i]) != before[i]:
                got[f"f{i}"] = _read(argv[i])
        if rec is not None:
            assert rec == got, f"{key}: the reference tool no longer gives the recorded answer (tests/golden/ref_tools.npz)"
        elif os.environ.get("RR_RECORD_REF_TOOLS") == "1":
            _load()[h] = got
            _save()
        return p
    if rec is None:
        pytest.fail(f"{os.path.basename(argv[0])} is not built here and this call was never recorded: {key}")
    for part, b in rec.items():
        if part.startswith("f"):
            with open(argv[int(part[1:])], "wb") as f:
                f.write(b)
    return subprocess.CompletedProcess(argv, json.loads(rec["meta"])["rc"], rec["stdout"], b"")


def check_call(argv):
    p = run(argv)
    if p.returncode:
        raise subprocess.CalledProcessError(p.returncode, argv, p.stdout, p.stderr)
    return 0


def check_output(argv):
    p = run(argv)
    if p.returncode:
        raise subprocess.CalledProcessError(p.returncode, argv, p.stdout, p.stderr)
    return p.stdout


def call(argv):
    return run(argv).returncode
