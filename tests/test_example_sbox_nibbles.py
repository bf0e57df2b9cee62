"""examples/encrypted_sbox_nibbles.py runs end to end on the GPU and its S-box outputs decrypt correctly."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_examples_sbox_is_the_aes_one():
    box = _load("encrypted_sbox_nibbles").aes_sbox()
    assert sorted(box) == list(range(256))
    assert [box[v] for v in (0x00, 0x01, 0x53, 0xFF)] == [0x63, 0x7C, 0xED, 0x16]  # FIPS 197, figure 7


@pytest.mark.gpu
def test_encrypted_sbox_nibbles_example():
    assert _load("encrypted_sbox_nibbles").main(["--bytes", "5"]) == 0
