"""examples/encrypted_ram.py runs end to end on the GPU: a 16-entry table of 4-bit words written and read by
encrypted addresses decrypts to the plaintext model."""
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
def test_encrypted_ram_example(capsys):
    assert _load("encrypted_ram").main(["--rounds", "2"]) == 0
    out = capsys.readouterr().out
    assert "k_rotate_chain<3>" in out and "Plaintext model" in out and "Success" in out
