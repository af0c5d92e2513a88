import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "reference: needs /root/reference (build container only)")


def pytest_collection_modifyitems(config, items):
    have_ref = os.path.isdir("/root/reference/fleetrl")
    skip_ref = pytest.mark.skip(reason="/root/reference is only present in the build container")
    for item in items:
        if "reference" in item.keywords and not have_ref:
            item.add_marker(skip_ref)


@pytest.fixture(scope="session")
def reference_inputs(tmp_path_factory):
    """A `data_path` holding the reference's input CSVs, unpacked once per session from tests/golden/inputs."""
    from golden_util import unpack_reference_inputs

    return unpack_reference_inputs(str(tmp_path_factory.mktemp("reference_inputs")))
