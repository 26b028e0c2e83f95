"""The `models` fixture, for the test modules that import it by name."""
import os
import tarfile

import pytest

import oracle_lib as ol


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """the reference's bundled models (cornell_box.obj and cornell/*.obj + .mtl, CC BY 3.0: see
    cornell/copyright.txt), stored as tests/golden/cornell_models.tar.gz and unpacked per run"""
    d = tmp_path_factory.mktemp("models")
    with tarfile.open(os.path.join(ol.ROOT, "tests", "golden", "cornell_models.tar.gz")) as t:
        if hasattr(tarfile, "data_filter"):
            t.extractall(d, filter="data")
        else:
            t.extractall(d)
    return str(d)
