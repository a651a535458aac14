import os
import shutil
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helpers import short_tmp_base  # noqa: E402


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a real MI355X GPU (run via gpurun)"
    )


@pytest.fixture
def tmp_socket_dir():
    """Short socket dir (unix socket paths are capped at ~107 chars).

    Not under tmp_path: pytest's base temp sits below $TMPDIR and adds the
    user and test names, which alone can exceed the cap."""
    d = tempfile.mkdtemp(prefix="dp-", dir=short_tmp_base())
    yield d
    shutil.rmtree(d, ignore_errors=True)
