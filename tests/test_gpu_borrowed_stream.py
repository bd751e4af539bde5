"""A context on a borrowed torch stream (zk_set_stream / zk_get_stream; see tests/_borrowed_stream_gpu.py, which runs in its own
process because it imports torch)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_borrowed_torch_stream():
    r = subprocess.run([sys.executable, os.path.join(HERE, "_borrowed_stream_gpu.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("STREAM-OK"), r.stdout[-3000:] + r.stderr[-4000:]
    assert "FAIL" not in r.stdout
