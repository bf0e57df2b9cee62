"""examples/encrypted_radix_add_fused.py runs end to end on the GPU and its sums decrypt correctly."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_encrypted_radix_add_fused_example():
    assert _load("encrypted_radix_add_fused").main(["--pairs", "3"]) == 0
