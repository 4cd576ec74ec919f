import os
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def orc():
    """The CPU oracle (test infrastructure; oracle/dd_oracle.h)."""
    from oracle import dd_oracle
    dd_oracle.lib()
    return dd_oracle


@pytest.fixture
def sock_dir():
    """A short directory for unix sockets: a socket's path holds at most 107 bytes, and pytest's tmp_path under a deep
    home or TMPDIR can be that long by itself."""
    d = tempfile.mkdtemp(prefix="dd_sock_", dir="/tmp" if os.access("/tmp", os.W_OK) else None)
    yield d
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


_ENGINES = {}


@pytest.fixture(scope="session")
def engine_factory(torch_cuda):
    """Engines are cached per (log2m, canonical): contexts keep their HBM workspaces."""
    from dandd_amd.engine import Engine

    def make(log2m=14, canonical=True):
        key = (log2m, canonical)
        if key not in _ENGINES:
            _ENGINES[key] = Engine(device=0, log2m=log2m, canonical=canonical)
        return _ENGINES[key]

    yield make
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
