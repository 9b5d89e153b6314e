"""The scope guards and the device scratch of the C++ host mirror (ssrlcv_amd/host/Scoped.hpp) through tests/cpp/scoped_test.cpp:
every entry condition of a Unity<float> of 5 values and of 1 for each of the three guards, two guards nested, a null argument and
the scratch.  The binary checks the contract at the top of the header and prints one "ok" line a case; the exact set of lines is
asserted here, so a case cannot go missing, and with the log switched on no guard may make Unity<T> warn."""
import os
import subprocess

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ENTRIES = ("cpu", "cpu-pinned", "gpu", "both-fore-cpu", "both-fore-gpu", "both-fore-both")
GUARDS = ("gpu-read", "gpu-write", "cpu-read")
WANT = (["ok %s %s n=%d" % (g, e, n) for n in (5, 1) for e in ENTRIES for g in GUARDS]
        + ["ok nested %s %s" % (g, e) for e in ("cpu", "gpu") for g in GUARDS]
        + ["ok null argument", "ok scratch", "done"])


def test_the_guards_and_the_scratch_keep_their_contract():
    host = os.path.join(H.ROOT, "ssrlcv_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host, "_build/scoped_test"])
    run = subprocess.run([os.path.join(host, "_build", "scoped_test")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                         env=dict(os.environ, SSRLCV_LOG="1"))
    out, err = run.stdout.decode(), run.stderr.decode()
    assert run.returncode == 0, out + err
    assert out.splitlines() == WANT, out + err
    assert "[warn]" not in err and "[error]" not in err, err
