"""examples/encrypted_6bit_table.py runs end to end on the GPU and its S-box outputs decrypt correctly."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_examples_sbox_is_des_s1():
    s1 = _load("encrypted_6bit_table").des_s1
    assert s1(0b011011) == 0b0101  # row 01, column 1101
    assert [s1(x) for x in (0, 1, 62, 63)] == [14, 0, 0, 13]
    for row in range(4):  # every row of a DES S-box is a permutation of 0 .. 15
        assert sorted(s1((row >> 1) << 5 | col << 1 | (row & 1)) for col in range(16)) == list(range(16))


@pytest.mark.gpu
def test_encrypted_6bit_table_example():
    assert _load("encrypted_6bit_table").main(["--items", "8"]) == 0
