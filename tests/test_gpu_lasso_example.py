"""examples/prescribe_from_csv.py --regression lasso runs end to end on its synthetic tracker file."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_prescribe_example_with_lasso(gpu_device, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "prescribe_from_csv.py"), "--regression", "lasso"],
                       capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "(regression: lasso)" in r.stdout
