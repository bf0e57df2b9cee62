"""examples/encrypted_sbox_packed.py runs end to end on the GPU and its outputs decrypt to the S-box's entries."""
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
def test_encrypted_sbox_packed_example(capsys):
    assert _load("encrypted_sbox_packed").main(["--queries", "2"]) == 0
    assert "16 CMUXes" in capsys.readouterr().out  # 2 queries x (1 + 7)
