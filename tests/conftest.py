import os
import sys

import pytest
import torch

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)

# The suite is self-contained: train(args) asks its datasets for
# download=True, which must neither reach for the network nor create
# directories outside the test's tmp_path.  Set in os.environ (not a
# fixture) so that the subprocesses the tests start inherit it.
os.environ["DDPX_OFFLINE"] = "1"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X GPU (run with -m gpu)")


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip_gpu = pytest.mark.skip(reason="no GPU in this environment")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip_gpu)


@pytest.fixture(autouse=True)
def _no_tqdm(monkeypatch):
    monkeypatch.setenv("DDPX_NO_TQDM", "1")
