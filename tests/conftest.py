import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sock_dir():
    """Short directory for AF_UNIX sockets.  sun_path holds 107 bytes and
    pytest's tmp_path (base temp + user + truncated test name) can exceed
    that, so sockets get a directory whose length does not depend on it."""
    import shutil
    import tempfile
    base = "/tmp" if os.access("/tmp", os.W_OK | os.X_OK) else None
    d = tempfile.mkdtemp(prefix="omq-", dir=base)
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture
def sock_dir():
    yield from _sock_dir()


@pytest.fixture(scope="module")
def sock_dir_module():
    yield from _sock_dir()


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a real MI355X GPU (run via gpurun)"
    )


def pytest_collection_modifyitems(config, items):
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if not has_gpu:
        skip = pytest.mark.skip(reason="no GPU in this container")
        for item in items:
            if "gpu" in item.keywords:
                item.add_marker(skip)
